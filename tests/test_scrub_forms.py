"""leoec_scrub_dev's persistent loop at test-sized batches: gf8_heal_list's
grid capped with LEOEC_SCRUB_GRID (measurement build), so that one workgroup
walks many items.

The product grid is min(objects x tiles, resident workgroups of the device):
on a test-sized batch every workgroup gets one item and never takes a second
trip.  With LEOEC_SCRUB_GRID=1 one workgroup walks every item of the list;
with 5 a workgroup's successive items change object, record and tile (5
divides neither the 3 tiles of an 8,704-byte block nor the 162 of a
164,992-byte one).  These are the cases in which a second trip of a workgroup
runs at all: state carried over from the previous item (its record, its
shards, its `full`: the position batch mixes objects whose output is the
ragged last block with objects whose blocks are all whole), an exit or a skip
not taken by the whole workgroup, and the barrier between two trips (the next
item's tables staged while a wave still reads this one's) can only go wrong
here.  Of the last the test is no proof: a build without that barrier passed
it on an MI355X (four dependent loads lie between a wave's last LDS read and
its next staging, more than the waves of a workgroup drift apart), so the
barrier is held by reading scrub_impl.hpp.  The expectations are
test_device_scrub.py's, byte for byte.

The measure_gpu tests need the measurement build's knob and run in a process
of their own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_scrub_forms_in_own_process below; in the product tests'
process they skip (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_scrub_forms.py -m measure_gpu
"""
import os
import subprocess
import sys

import pytest

import locate_helpers as L
import scrub_dev_helpers as D
import scrub_helpers as S

FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 10, 4, 8, 164992), ("vandrs", 16, 4, 8, 8704)]
GRIDS = ("1", "5", None)


def test_families_and_grids():
    assert all(f in L.FAMILIES for f in FAMILIES)
    for cls, k, m, w, B in FAMILIES:
        tiles = -(-B // (1024 if B > 160 * 1024 else 4096))
        assert tiles in (3, 162) and tiles % 5 != 0
        assert (k + m) * tiles > 5  # more items than workgroups: every one loops


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", FAMILIES, ids=L.family_id)
def test_scrub_grid_caps(gpu, le, oracle, family, measure):
    cls, k, m, w, B = family
    errors = []
    for grid in GRIDS:
        if grid is None:
            measure.delenv("LEOEC_SCRUB_GRID")
        else:
            measure.setenv("LEOEC_SCRUB_GRID", grid)
        for case in D.SCRUB.cases(le, oracle, family):
            dmg, _, locate = S.position_batch(case)
            want = S.two_block_word(oracle, le, case, dmg, locate)
            assert want[-1] == S.MANY  # m = 4: every word by construction
            work, par = L.damaged_arenas(gpu, case, dmg)
            errors += [f"LEOEC_SCRUB_GRID={grid}: {e}"
                       for e in D.SCRUB.check_scrub(gpu, le, case, work, par, want)[1]]
            dmg, want = D.dense_batch(case)
            work, par = L.damaged_arenas(gpu, case, dmg)
            errors += [f"LEOEC_SCRUB_GRID={grid} dense: {e}"
                       for e in D.SCRUB.check_scrub(gpu, le, case, work, par, want)[1]]
        # every valid byte of block b damaged in object b: every item's stores are needed
        for case in D.SCRUB.whole_cases(le, oracle, family):
            blocks = S.whole_batch(case)
            work, par = S.whole_arenas(gpu, case, blocks)
            errors += [f"LEOEC_SCRUB_GRID={grid} whole blocks: {e}" for e in
                       D.SCRUB.check_scrub(gpu, le, case, work, par, S.whole_words(case, blocks))[1]]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_scrub_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu tests of this file in a child process that loads
    libleoec_measure.so alone (as test_heal_forms.py's
    test_heal_forms_in_own_process).  The child's output goes to
    scrub_forms.log in the test's temporary directory; a failure shows its
    tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "scrub_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"scrub form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
