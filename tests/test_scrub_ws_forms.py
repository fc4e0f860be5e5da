"""leoec_scrub_ws_dev's persistent loop at test-sized batches: bit_heal_list's
grid capped with LEOEC_SCRUB_GRID (measurement build), so that one workgroup
walks many items.

The product grid is min(objects x tiles, resident workgroups of the device):
on a test-sized batch every workgroup gets one item and never takes a second
trip, so this is the only place where the loop is tested.  With
LEOEC_SCRUB_GRID=1 one workgroup walks every item of the list; with 7 a
workgroup's successive items change object, record and tile (7 divides none of
the tile counts, 5, 3 and 9 tiles of 1 KiB in a packet of 4,352, 2,176 and
8,704 bytes, and lies below every family's item count).  What can only go
wrong on a second trip: state carried over from the previous item (its
accumulators, which are zeroed per item, its record, its `full`: the position
batch mixes objects whose lost block is the ragged last data block with
objects whose blocks are all whole) and a skip not taken by the whole wave.
The sizes are test_device_scrub_ws.py's three (scrub_dev_helpers.SCRUB_WS.sizes): at
k B - 1 and k B a workgroup's successive items alternate between whole tiles
(the unguarded loads and stores) and a packet's last, partial tile (the guarded
ones).  The expectations are test_device_scrub_ws.py's, byte for byte.

The measure_gpu tests need the measurement build's knob and run in a process
of their own that loads libleoec_measure.so alone (LEOEC_LIBRARY=measure),
started by test_scrub_ws_forms_in_own_process below; in the product tests'
process they skip (the `measure` fixture).
Run directly: LEOEC_LIBRARY=measure python -m pytest tests/test_scrub_ws_forms.py -m measure_gpu
"""
import os
import re
import subprocess
import sys

import pytest

import locate_ws_helpers as W
import scrub_dev_helpers as D
import scrub_helpers as S

X = D.SCRUB_WS

FAMILIES = [("cauchyrs", 10, 4, 8, 4352 * 8), ("liberation", 4, 2, 7, 2176 * 7),
            ("cauchyrs", 5, 3, 17, 8704 * 17)]
CAP = 7
GRIDS = ("1", str(CAP), None)


def kernel_tile():
    """The tile width bit_heal_list really has: kBitHealLanes x 16 bytes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "leo_erasure_amd", "csrc", "bit_heal_tile.hpp")) as f:
        text = f.read()
    lanes = int(re.search(r"constexpr int kBitHealLanes = (\d+);", text).group(1))
    assert re.search(r"constexpr uint32_t kBitHealTile = kBitHealLanes \* 16u;", text)
    return lanes * 16


def test_families_and_grids():
    tile = kernel_tile()
    assert tile == X.TILE
    assert all(f in W.FAMILIES for f in FAMILIES)
    counts = []
    for cls, k, m, w, B in FAMILIES:
        tiles = -(-(B // w) // tile)
        counts.append(tiles)
        assert tiles % CAP != 0 and CAP % tiles != 0, (cls, tiles)
        # the fewest items any batch of the family lists: the position batch
        # names k + m objects at the first size, the dense batch more
        assert (k + m) * tiles > CAP
    assert counts == [5, 3, 9]


@pytest.mark.gpu
@pytest.mark.measure_gpu
@pytest.mark.parametrize("family", FAMILIES, ids=W.family_id)
def test_scrub_ws_grid_caps(gpu, le, oracle, family, measure):
    import locate_helpers as L
    cls, k, m, w, B = family
    errors = []
    for grid in GRIDS:
        if grid is None:
            measure.delenv("LEOEC_SCRUB_GRID")
        else:
            measure.setenv("LEOEC_SCRUB_GRID", grid)
        for case in X.cases(le, oracle, family):
            dmg, _, locate = S.position_batch(case)
            want = S.two_block_word(oracle, le, case, dmg, locate)
            skip = None if want[-1] == S.MANY else case.n - 1
            assert skip is None or m == 2
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
def test_scrub_ws_forms_in_own_process(gpu, tmp_path):
    """The measure_gpu tests of this file in a child process that loads
    libleoec_measure.so alone (as test_scrub_forms.py's
    test_scrub_forms_in_own_process).  The child's output goes to
    scrub_ws_forms.log in the test's temporary directory; a failure shows its
    tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.skip("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    log = str(tmp_path / "scrub_ws_forms.log")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1")
    cmd = [sys.executable, "-u", "-m", "pytest", os.path.abspath(__file__),
           "-m", "measure_gpu", "-x", "-q", "-p", "no:cacheprovider",
           "--timeout", "120", "--timeout-method", "thread"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                             timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"scrub_ws form tests failed (rc {rc}), {log}:\n{tail}"
    summary = tail.strip().splitlines()[-1]
    assert "passed" in summary and "skipped" not in summary, summary
