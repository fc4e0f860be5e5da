"""leoec_scrub_gfw_dev's persistent loop at test-sized batches: gfw_heal_list's
grid capped with LEOEC_SCRUB_GRID (measurement build), so that one workgroup
walks many items.

The product grid is min(objects x tiles, resident workgroups of the device):
on a test-sized batch every workgroup gets one item and never takes a second
trip (test_device_scrub_gfw.py's batch of twice the grid aside), so this is
where the loop is tested at every width.  With LEOEC_SCRUB_GRID=1 one
workgroup walks every item of the list; with 7 a workgroup's successive items
change object, record and tile (7 is no multiple of any tile count, 3 tiles of
4 KiB in a block of 8,704 bytes and 1 at the one-tile size, and lies below
every batch's item count).  What can only go wrong on a second trip: state
carried over from the previous item (the accumulator row, which is zeroed per
item, the record, `full`: the position batch mixes objects whose lost block is
the ragged last data block with objects whose blocks are all whole) and a skip
not taken by the whole wave (an empty lost block, a tile past a short block).
One family per width, at test_device_scrub_gfw.py's three sizes; the
expectations are that module's, byte for byte.

The measure_gpu tests need the measurement build's knob and run in a process
of their own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_scrub_gfw_forms_in_own_process below; in the product tests'
process they skip (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_scrub_gfw_forms.py -m measure_gpu
"""
import os
import subprocess
import sys

import pytest

import locate_gfw_helpers as G
import scrub_dev_helpers as D
import scrub_helpers as S

X = D.SCRUB_GFW

FAMILIES = [("vandrs", 20, 4, 8, 8704), ("vandrs", 10, 4, 16, 8704), ("vandrs", 6, 3, 32, 8704)]
CAP = 7
GRIDS = ("1", str(CAP), None)


def test_families_and_grids(le):
    assert all(f in X.FAMILIES for f in FAMILIES) and sorted(f[3] for f in FAMILIES) == [8, 16, 32]
    for family in FAMILIES:
        cls, k, m, w, B = family
        counts = []
        for size in X.sizes(family):
            bs, _ = le.layout(cls, (k, m, w), size)
            tiles = -(-bs // X.TILE)
            counts.append(tiles)
            assert tiles % CAP != 0, (family, size, tiles)
            # the fewest items any batch lists: the position and whole-block
            # batches name every block with a valid byte once
            named = sum(1 for b in range(k + m) if b >= k or b * bs < size)
            assert named * tiles > CAP, (family, size, named, tiles)
        assert counts == [3, 1, 3]


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", FAMILIES, ids=G.family_id)
def test_scrub_gfw_grid_caps(gpu, le, oracle, family, measure):
    import locate_helpers as L
    errors = []
    for grid in GRIDS:
        if grid is None:
            measure.delenv("LEOEC_SCRUB_GRID")
        else:
            measure.setenv("LEOEC_SCRUB_GRID", grid)
        for case in X.cases(le, oracle, family):
            dmg, want, skip = X.position(le, oracle, case)
            work, par = L.damaged_arenas(gpu, case, dmg)
            errors += [f"LEOEC_SCRUB_GRID={grid}: {e}"
                       for e in X.check_scrub(gpu, le, case, work, par, want, skip)[1]]
            dmg, want = D.dense_batch(case)
            work, par = L.damaged_arenas(gpu, case, dmg)
            errors += [f"LEOEC_SCRUB_GRID={grid} dense: {e}"
                       for e in X.check_scrub(gpu, le, case, work, par, want)[1]]
        # every valid byte of block b damaged in object b: every item's stores are needed
        for case in X.whole_cases(le, oracle, family):
            blocks = S.whole_batch(case)
            work, par = S.whole_arenas(gpu, case, blocks)
            errors += [f"LEOEC_SCRUB_GRID={grid} whole blocks: {e}" for e in
                       X.check_scrub(gpu, le, case, work, par, S.whole_words(case, blocks))[1]]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_scrub_gfw_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu tests of this file in a child process that loads
    libleoec_measure.so alone (as test_scrub_ws_forms.py's
    test_scrub_ws_forms_in_own_process).  The child's output goes to
    scrub_gfw_forms.log in the test's temporary directory; a failure shows its
    tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "scrub_gfw_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"scrub_gfw form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
