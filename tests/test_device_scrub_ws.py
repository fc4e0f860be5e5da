"""leoec_scrub_ws_dev on the device (product library): locate_ws and heal in
one call for cauchyrs and liberation, on the edge harness of gpu_helpers
(guarded arenas, random non-zero bytes behind every object, every byte of both
arenas, the words around the covered ones and the workspace's tail compared
after every call).

The contract is the composition device.locate_ws then device.heal(lost =
report); the batches are test_device_scrub.py's (scrub_helpers' position batch:
object b of k + m + 2 has block b damaged, one object is clean, one has two
damaged blocks; a clean batch; scrub_dev_helpers' dense batch), for the six
bitmatrix families of locate_ws_helpers.FAMILIES at the sizes k B - 1 and
16 w (k - 2) + 5 (every packet has whole 1 KiB tiles and a last partial one,
the last data block is ragged at the first size, empty with the one before it
ragged at the second) and at k B, where no block is clipped
(scrub_dev_helpers.SCRUB_WS.sizes).  Expected words are by construction.

Those batches damage at most 64 bytes of a block, 64 / w of a packet, all in
lane 0's column of one tile: every other byte equals the snapshot whether
bit_heal_list stored it or not.  The whole-block batch
(scrub_helpers.whole_batch, held against the oracle and the host model by
test_scrub_whole_cpu.py) damages every valid byte of block b in object b: the
result is right only if every tile of every packet, every lane, both store
paths and the ragged tail were written.  The dense form of it in a batch of
twice the launch's grid runs the kernel's loop into its second trip in the
product library."""
import os
import re
import subprocess
import sys

import pytest

import gpu_helpers as H
import locate_helpers as L
import locate_ws_helpers as W
import scrub_dev_helpers as D
import pending_helpers as PE
import scrub_helpers as S
import stream_helpers as T

X = D.SCRUB_WS


@pytest.fixture(scope="module", params=X.FAMILIES, ids=X.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


# every family's packet has whole 1 KiB tiles and a last partial one
assert all(B // w > X.TILE and (B // w) % X.TILE != 0 for _, _, _, w, B in W.FAMILIES)


@pytest.mark.gpu
def test_device_scrub_ws_positions(gpu, le, oracle, family):
    """One scrub of the position batch: the by-construction report between
    intact sentinels, totals, every named object back to the snapshot, the
    two-block object untouched.  Then the same damage through device.locate_ws
    + device.heal: identical arenas and words, no object left out.  Then a
    second scrub of the healed arenas: all zero but for the two-block object,
    nothing rebuilt, no byte changed."""
    errors = []
    for case in X.cases(le, oracle, family):
        dmg, want, skip = X.position(le, oracle, case)
        work, par = L.damaged_arenas(gpu, case, dmg)
        errors += X.check_scrub(gpu, le, case, work, par, want, skip)[1]
        work, par, got, _, errs = X.check_equivalence(gpu, le, case, dmg)
        errors += errs
        if got != want:
            errors.append(f"{case.ident()}: equivalence run's report {[hex(x) for x in got]}")
        healed, par_healed = work.clone(), par.clone()
        _, again, tot, errs = X.run_scrub(gpu, le, case, work, par)
        errors += errs
        ctx = f"second scrub_ws {case.ident()} bs {case.bs}"
        # (m = 2 with a third block named: the other k + 1 blocks fit one
        # another, so the rebuilt stripe is consistent, if wrong)
        many = 1 if want[-1] == S.MANY else 0
        expect = [0] * (case.n - 1) + [S.MANY if many else 0]
        if again != expect or tot != [0, many]:
            errors.append(f"{ctx}: report {[hex(x) for x in again]}, totals {tot}, expected "
                          f"{[hex(x) for x in expect]}, {[0, many]}")
        for err in (H.arena_diff(gpu, work, healed, case.guard, f"{ctx}: objs"),
                    H.arena_diff(gpu, par, par_healed, 1, f"{ctx}: parity")):
            if err:
                errors.append(err)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_ws_clean_batch(gpu, le, oracle, family):
    """Nothing damaged: every word 0, totals (0, 0), no byte written."""
    errors = []
    for case in X.cases(le, oracle, family):
        work, par = L.damaged_arenas(gpu, case, [])
        errors += X.check_scrub(gpu, le, case, work, par, [0] * case.n)[1]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_ws_dense_batch(gpu, le, oracle, family):
    """Every object with one damaged block, object o block o mod (k + m): every
    one named and rebuilt, and the two-call sequence leaves the same bytes."""
    errors = []
    for case in X.cases(le, oracle, family):
        dmg, want = D.dense_batch(case)
        work, par = L.damaged_arenas(gpu, case, dmg)
        errors += X.check_scrub(gpu, le, case, work, par, want)[1]
        errors += X.check_equivalence(gpu, le, case, dmg)[4]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_ws_small_workspaces(gpu, le, oracle, family):
    """The position batch with the minimum workspace (one object per chunk)
    and with room for 3 objects: report, totals and arenas as with one pass."""
    errors = []
    for case in X.cases(le, oracle, family):
        dmg, want, skip = X.position(le, oracle, case)
        ref_work, ref_par, ref_got, ref_tot, errs = X.check_equivalence(gpu, le, case, dmg)
        errors += errs
        for room in (1, 3):
            work, par = L.damaged_arenas(gpu, case, dmg)
            errors += X.check_scrub(gpu, le, case, work, par, want, skip, room=room)[1]
            work, par = L.damaged_arenas(gpu, case, dmg)
            _, got, tot, errs = X.run_scrub(gpu, le, case, work, par, room=room)
            errors += errs
            ctx = f"scrub_ws {case.ident()} bs {case.bs} room {room} against one pass"
            if got != ref_got or tot != ref_tot:
                errors.append(f"{ctx}: report {[hex(x) for x in got]}, totals {tot}")
            for err in (H.arena_diff(gpu, work, ref_work, case.guard, f"{ctx}: objs"),
                        H.arena_diff(gpu, par, ref_par, 1, f"{ctx}: parity")):
                if err:
                    errors.append(err)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_ws_whole_blocks(gpu, le, oracle, family):
    """Object b has every valid byte of block b damaged: one scrub_ws, and one
    beside device.locate_ws + device.heal, both back to the snapshot byte for
    byte; the rebuild was bit_heal_list's (the list in the workspace).  Then
    once more with room for one object in the workspace."""
    errors = []
    for case in X.whole_cases(le, oracle, family):
        blocks = S.whole_batch(case)
        path, errs = X.check_whole(gpu, le, case, blocks)
        errors += errs
        if path != "list":
            errors.append(f"{case.ident()}: not the kernel path (more than 16 block tables in this "
                          f"process?): {path}")
        work, par = S.whole_arenas(gpu, case, blocks)
        errors += ["whole blocks: " + e for e in
                   X.check_scrub(gpu, le, case, work, par, S.whole_words(case, blocks), room=1)[1]]
    assert not errors, "\n".join(errors[:20])


# bit_heal_list's grid, restated: compute units x resident workgroups
# (bit_heal_tile.hpp: one wave each, 32 waves a compute unit, w KiB of its
# 160 KiB of LDS each)
# (m = 3: neither side builds an m = 2 Cauchy matrix past w = 20)
# (scrub_dev_helpers.SCRUB_WS.resident)
LARGE = ("cauchyrs", 2, 3, 32, 1040 * 32)  # packets of 1,040 bytes: a full tile and a 16-byte one


def test_grid_constants_are_the_sources(le, oracle):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "leo_erasure_amd", "csrc")
    with open(os.path.join(csrc, "bit_heal_tile.hpp")) as fh:  # the constants and resident()
        text = fh.read()
    with open(os.path.join(csrc, "scrub_bit_impl.hpp")) as fh:  # the launcher
        launch = fh.read()
    with open(os.path.join(csrc, "heal_impl.hpp")) as fh:  # list_grid
        heal = fh.read()
    assert re.findall(r"constexpr int kBitHealLanes = (\d+);", text) == ["64"]
    assert "constexpr uint32_t kBitHealTile = kBitHealLanes * 16u;" in text and X.TILE == 64 * 16
    assert re.search(r"inline uint32_t bit_heal_list_resident\(uint32_t w\) \{\s*"
                     r"const uint32_t by_lds = 160u / w;[^\n]*\n\s*"
                     r"return by_lds < 32u \? by_lds : 32u;\s*\}", text)
    assert ("const uint32_t grid = list_grid((uint64_t)a.h.nobj * a.h.tiles, bit_heal_list_resident(a.w), cap);"
            in launch)
    assert "uint64_t grid = (uint64_t)device_cus() * resident;" in heal
    assert "grid = grid < all ? grid : all;" in heal
    assert [X.resident(w) for w in (2, 5, 6, 17, 32)] == [32, 32, 26, 9, 5]
    cls, k, m, w, B = LARGE
    assert B % (16 * w) == 0 and -(-(B // w) // X.TILE) == 2 and W.served(cls, k, m, w)
    assert len(oracle.encode(cls, k, m, w, b"\x5a")) == k + m
    assert le.device.scrub_ws_workspace(cls, (k, m, w), k * B - 1, 1) == 32 + m * B


@pytest.mark.gpu
def test_device_scrub_ws_batch_larger_than_the_grid(gpu, le, oracle):
    """The dense whole-block batch with objects x tiles at least twice
    bit_heal_list's grid: every workgroup takes a second item
    (`item += gridDim.x`) in the product library, at w = 32 (5 resident
    workgroups a compute unit, 32 KiB of LDS each).  Every object against the
    oracle's snapshot."""
    cls, k, m, w, B = LARGE
    cus = gpu.cuda.get_device_properties(gpu.cuda.current_device()).multi_processor_count
    tiles = -(-(B // w) // X.TILE)
    n = -(-2 * cus * X.resident(w) // tiles)
    grid = X.grid(cus, n, tiles, 0, w)
    case = H.EdgeCase(le, oracle, LARGE[:4], k * B - 1, n)
    assert case.bs == B and n * tiles >= 2 * grid and grid == cus * X.resident(w)
    blocks = S.whole_dense_batch(case)
    want = S.whole_words(case, blocks)
    assert all(x == 1 << (o % (k + m)) for o, x in enumerate(want))  # no object left out
    work, par = S.whole_arenas(gpu, case, blocks)
    keep = []
    errors = X.check_scrub(gpu, le, case, work, par, want, keep=keep)[1]
    assert not errors, "\n".join(e[:2000] for e in errors[:20])
    assert D.path(gpu, keep[0], want) == "list"


@pytest.mark.gpu
def test_device_scrub_ws_forwards_the_fused_family(gpu, le, oracle):
    """vandrs(10,4,8) through device.scrub_ws equals device.scrub: report,
    totals and arenas."""
    family = ("vandrs", 10, 4, 8, 8704)
    assert family in L.FAMILIES
    errors = []
    for case in X.cases(le, oracle, family):
        dmg, want, skip = X.position(le, oracle, case)
        assert skip is None
        work, par = L.damaged_arenas(gpu, case, dmg)
        errors += X.check_scrub(gpu, le, case, work, par, want)[1]
        work, par = L.damaged_arenas(gpu, case, dmg)
        work2, par2 = work.clone(), par.clone()
        _, got, tot, errs = X.run_scrub(gpu, le, case, work, par)
        errors += errs
        _, got2, tot2, errs = D.SCRUB.run_scrub(gpu, le, case, work2, par2)
        errors += errs
        ctx = f"scrub_ws against scrub {case.ident()}"
        if (got, tot) != (got2, tot2):
            errors.append(f"{ctx}: report {[hex(x) for x in got]} {tot}, scrub's "
                          f"{[hex(x) for x in got2]} {tot2}")
        for err in (H.arena_diff(gpu, work, work2, case.guard, f"{ctx}: objs"),
                    H.arena_diff(gpu, par, par2, 1, f"{ctx}: parity")):
            if err:
                errors.append(err)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_ws_captured(gpu, le, oracle):
    """The call is memsets and launches on the stream: captured into a graph
    (after one plain call, which builds the block table and loads the code
    objects) it replays to the same report, totals and arenas, and again after
    the buffers are refilled with a differently damaged batch."""
    family = X.FAMILIES[0]
    assert family[:4] == ("cauchyrs", 10, 4, 8)
    case = next(iter(X.cases(le, oracle, family)))
    dmg, want, skip = X.position(le, oracle, case)
    assert skip is None  # m >= 3: every word by construction
    first = L.damaged_arenas(gpu, case, dmg)
    errors = X.check_scrub(gpu, le, case, first[0].clone(), first[1].clone(), want)[1]
    assert not errors, "\n".join(errors)
    dense, dense_words = D.dense_batch(case)
    second = L.damaged_arenas(gpu, case, dense)
    b = D.Buffers(X, gpu, le, case)
    cap = T.Captured(gpu, b.call, lambda: b.refill(first), lambda: b.untouched(first))
    errors = cap.errors
    for r, (before, words) in enumerate(((first, want), (second, dense_words), (first, want))):
        b.refill(before)
        cap.replay()
        errors += b.check(before, words, f"captured scrub_ws {case.ident()} replay {r}")
    assert not errors, "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# A HIP error pending on the calling thread (test_pending_hip_error.py's way:
# hipSetDevice(-1) through the library's own runtime handle, no torch call
# between planting and the clear).

@pytest.mark.gpu
def test_device_scrub_ws_with_pending_error(gpu, le, oracle):
    """A first plain call, then one with hipErrorInvalidDevice pending on the
    thread: LEOEC_OK, the results right, the same code in the slot afterwards."""
    cls, k, m, w = "cauchyrs", 6, 3, 4
    B = (4096 // (16 * w) + 1) * 16 * w
    case = H.edge_case(le, oracle, (cls, k, m, w), k * B - 17, n=3)
    dmg, want = D.dense_batch(case)
    work, par = L.damaged_arenas(gpu, case, dmg)
    first = X.check_scrub(gpu, le, case, work, par, want)[1]
    assert not first, "\n".join(first)
    dmg = [e for o in range(3) for e in S._entries(case, o, k + o, S.VALUES[:S.HITS])]
    want = [1 << (k + o) for o in range(3)]
    work, par = L.damaged_arenas(gpu, case, dmg)
    calls = []
    with PE.planted(gpu, le, calls, "leoec_scrub_ws_dev") as rt:
        errors = X.check_scrub(gpu, le, case, work, par, want)[1]
    assert calls == [(0, PE.HIP_ERROR_INVALID_DEVICE)], calls
    assert not errors, "\n".join(errors)
    assert rt.hipPeekAtLastError() == PE.HIP_SUCCESS


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_scrub_ws_with_full_table_cache_in_own_process(gpu, tmp_path):
    """tests/scrub_table_cache_child.py scrub_ws in a fresh process: 16 bitmatrix
    configurations scrubbed first fill the block table cache, the scrub of a
    17th then takes the composed path and must still equal locate_ws + heal
    byte for byte."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = str(tmp_path / "scrub_ws_table_cache.log")
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    cmd = [sys.executable, "-u", os.path.join(root, "tests", "scrub_table_cache_child.py"), "scrub_ws"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT, timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"scrub_table_cache_child.py scrub_ws failed (rc {rc}), {log}:\n{tail}"
    assert "17th configuration scrubbed" in tail, tail
