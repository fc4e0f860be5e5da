"""leoec_scrub_dev on the device (product library): locate and heal in one
call, on the edge harness of gpu_helpers (guarded arenas, random non-zero
bytes behind every object, every byte of both arenas, the words around the
covered ones and the workspace's tail compared after every call).

The contract is the composition device.locate then device.heal(lost = report);
the batches are scrub_helpers' position batch (object b of k + m + 2 has block
b damaged, one object is clean, one has two damaged blocks), a clean batch and
a dense batch (object o has block o mod (k + m) damaged), for the six families
of locate_helpers.FAMILIES (the fused configurations at 256 lanes, the 64-lane
tiles, K = 16) at the sizes k B - 1 and 16 w (k - 2) + 5.  Expected words are
by construction (scrub_helpers.position_batch, held against the oracle and the
host model by test_device_scrub_positions.py's CPU test).

Those batches damage at most 64 bytes of a block, so every other byte of it
equals the snapshot whether gf8_heal_list stored it or not.  The whole-block
batch (scrub_helpers.whole_batch, held against the oracle and the host model by
test_scrub_whole_cpu.py) damages every valid byte of block b in object b: the
result is right only if every tile, every lane, both store paths and the ragged
tail were written.  The dense form of it in a batch of twice the launch's grid
runs the kernel's loop into its second trip in the product library."""
import os
import re
import subprocess
import sys

import pytest

import gpu_helpers as H
import locate_helpers as L
import scrub_dev_helpers as D
import scrub_helpers as S
import stream_helpers as T

X = D.SCRUB


@pytest.fixture(scope="module", params=X.FAMILIES, ids=X.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def test_family_table():
    assert X.FAMILIES is L.FAMILIES and len(L.FAMILIES) == 6
    assert ("vandrs", 10, 4, 8, 164992) in L.FAMILIES and ("vandrs", 16, 4, 8, 8704) in L.FAMILIES
    assert any(f[2] == 2 for f in L.FAMILIES)  # the m = 2 limit is met


@pytest.mark.gpu
def test_device_scrub_positions(gpu, le, oracle, family):
    """One scrub of the position batch: the by-construction report between
    intact sentinels, totals, every named object back to the snapshot, the
    two-block object untouched.  Then the same damage through device.locate +
    device.heal: identical arenas and words, no object left out.  Then a second
    scrub of the healed arenas: all zero but for the two-block object, nothing
    rebuilt, no byte changed."""
    errors = []
    for case in X.cases(le, oracle, family):
        dmg, want, skip = X.position(le, oracle, case)
        work, par = L.damaged_arenas(gpu, case, dmg)
        errors += X.check_scrub(gpu, le, case, work, par, want, skip)[1]
        work, par, got, _, errs = X.check_equivalence(gpu, le, case, dmg)
        errors += errs
        if got != want:
            errors.append(f"{case.ident()}: equivalence run's report {[hex(x) for x in got]}")
        # the healed arenas again
        healed, par_healed = work.clone(), par.clone()
        _, again, tot, errs = X.run_scrub(gpu, le, case, work, par)
        errors += errs
        ctx = f"second scrub {case.ident()} bs {case.bs}"
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
def test_device_scrub_clean_batch(gpu, le, oracle, family):
    """Nothing damaged: every word 0, totals (0, 0), no byte written."""
    errors = []
    for case in X.cases(le, oracle, family):
        work, par = L.damaged_arenas(gpu, case, [])
        errors += X.check_scrub(gpu, le, case, work, par, [0] * case.n)[1]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_dense_batch(gpu, le, oracle, family):
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
def test_device_scrub_whole_blocks(gpu, le, oracle, family):
    """Object b has every valid byte of block b damaged: one scrub, and one
    beside device.locate + device.heal, both back to the snapshot byte for
    byte; the rebuild was gf8_heal_list's (the list in the workspace)."""
    errors = []
    for case in X.whole_cases(le, oracle, family):
        path, errs = X.check_whole(gpu, le, case, S.whole_batch(case))
        errors += errs
        if path != "list":
            errors.append(f"{case.ident()}: not the kernel path (more than 16 heal tables in this "
                          f"process?): {path}")
    assert not errors, "\n".join(errors[:20])


# gf8_heal_list's grid, restated (scrub_dev_helpers.SCRUB.resident): compute
# units x resident workgroups (scrub_impl.hpp: 4 SIMDs of kGf8HealWaves waves,
# wg / 64 waves a workgroup)
GF8_HEAL_WAVES = 4
LARGE = ("vandrs", 4, 2, 8, 4224)  # 256 lanes: a full 4,096-byte tile and a 128-byte one


def test_grid_constants_are_the_sources():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "leo_erasure_amd", "csrc")
    with open(os.path.join(csrc, "heal_impl.hpp")) as fh:
        heal = fh.read()
    with open(os.path.join(csrc, "scrub_impl.hpp")) as fh:
        scrub = fh.read()
    assert re.findall(r"#define LEOEC_GF8_HEAL_WAVES (\d+)", heal) == [str(GF8_HEAL_WAVES)]
    assert "constexpr int kGf8HealWaves = LEOEC_GF8_HEAL_WAVES;" in heal
    assert ("inline uint32_t gf8_heal_list_resident(uint32_t wg) "
            "{ return 4u * (uint32_t)kGf8HealWaves * 64u / wg; }") in scrub
    # the grid rule: list_grid, the one function every list kernel's launcher calls
    assert ("const uint32_t grid = list_grid((uint64_t)a.nobj * a.tiles, gf8_heal_list_resident(wg), cap);"
            in scrub)
    assert re.search(r"inline uint32_t list_grid\(uint64_t all, uint32_t resident, uint32_t cap\) \{\s*"
                     r"uint64_t grid = \(uint64_t\)device_cus\(\) \* resident;\s*"
                     r"grid = grid < all \? grid : all;\s*"
                     r"if \(cap != 0u && grid > cap\) grid = cap;\s*"
                     r"return \(uint32_t\)grid;\s*\}", heal)
    assert [X.resident(wg) for wg in (256, 64)] == [4 * GF8_HEAL_WAVES * 64 // 256, 4 * GF8_HEAL_WAVES] == [4, 16]
    cls, k, m, w, B = LARGE
    assert B <= 160 * 1024 and -(-B // 4096) == 2  # the 256-lane form, two tiles a block


@pytest.mark.gpu
def test_device_scrub_batch_larger_than_the_grid(gpu, le, oracle):
    """The dense whole-block batch with objects x tiles at least twice
    gf8_heal_list's grid: every workgroup takes a second item
    (`item += gridDim.x`) in the product library.  Every object against the
    oracle's snapshot."""
    cls, k, m, w, B = LARGE
    cus = gpu.cuda.get_device_properties(gpu.cuda.current_device()).multi_processor_count
    tiles = -(-B // X.TILE)
    n = -(-2 * cus * X.resident(256) // tiles)
    grid = X.grid(cus, n, tiles, 0, 256)
    case = H.EdgeCase(le, oracle, LARGE[:4], k * B - 1, n)
    assert case.bs == B and n * tiles >= 2 * grid and grid == cus * X.resident(256)
    blocks = S.whole_dense_batch(case)
    want = S.whole_words(case, blocks)
    assert all(x == 1 << (o % (k + m)) for o, x in enumerate(want))  # no object left out
    work, par = S.whole_arenas(gpu, case, blocks)
    keep = []
    errors = X.check_scrub(gpu, le, case, work, par, want, keep=keep)[1]
    assert not errors, "\n".join(e[:2000] for e in errors[:20])
    assert D.path(gpu, keep[0], want) == "list"


@pytest.mark.gpu
def test_device_scrub_captured(gpu, le, oracle):
    """The call is memsets and launches on the stream, a linear chain: captured
    into a graph (after one plain call, which builds heal's table and loads
    the code objects) it replays to the same report, totals and arenas, and
    again after the buffers are refilled with a differently damaged batch."""
    case = next(iter(X.cases(le, oracle, X.FAMILIES[0])))
    dmg, want, skip = X.position(le, oracle, case)
    assert skip is None and want[-1] == S.MANY  # m >= 3: every word by construction
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
        errors += b.check(before, words, f"captured scrub {case.ident()} replay {r}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("call", D.CALLS, ids=lambda c: c.name)
def test_harness_reports_a_wrong_word_and_an_unexpected_object(gpu, le, oracle, call):
    """check_scrub must fail when it should.  The position batch of the call's
    first family at 16 w (k - 2) + 5 through a correct call, (a) against
    expectations with one word changed to a single-bit word: the two-block
    object's, so the object shows in the report, in the totals and, left as it
    was damaged where the expectations have it rebuilt, in both arenas; and
    one rebuilt object's, to another block: the report alone, since the counts
    and the bytes are the same; (b) with the clean object damaged as well,
    which the expectations do not know: a report error naming it."""
    family = call.FAMILIES[0]
    cls, k, m, w, B = family
    case = next(iter(call.cases(le, oracle, family, [16 * w * (k - 2) + 5])))
    n, two = case.n, case.n - 1
    dmg, want, skip = call.position(le, oracle, case)
    assert n == k + m + 2 and skip is None
    assert want[1] == 2 and want[k + m] == 0 and want[two] == S.MANY and D.counts(want) == [k + m - 1, 1]

    def errors_of(dmg, words):
        work, par = L.damaged_arenas(gpu, case, dmg)
        return call.check_scrub(gpu, le, case, work, par, words)[1]

    assert errors_of(dmg, want) == []
    # (a) the two-block object expected with block 0 named and rebuilt
    errors = errors_of(dmg, want[:two] + [1])
    assert len(errors) == 4, errors
    assert f"{call.name} {case.ident()}" in errors[0] and f"objects [{two}]: report" in errors[0]
    assert f"totals [{k + m - 1}, 1], expected [{k + m}, 0]" in errors[1]
    assert ": objs: " in errors[2] and f"in rows [{two}] " in errors[2]
    assert ": parity: " in errors[3] and f"in rows [{two}] " in errors[3]
    # object 1 expected with block 2 named: the same counts, the same bytes
    errors = errors_of(dmg, [want[0], 4] + want[2:])
    assert len(errors) == 1 and "objects [1]: report" in errors[0], errors
    # (b) the clean object k + m has block 0 damaged too
    errors = errors_of(dmg + S._entries(case, k + m, 0, S.VALUES[:S.HITS]), want)
    assert len(errors) == 2, errors
    assert f"objects [{k + m}]: report" in errors[0]
    assert f"totals [{k + m}, 1], expected [{k + m - 1}, 1]" in errors[1]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_scrub_with_full_table_cache_in_own_process(gpu, tmp_path):
    """tests/scrub_table_cache_child.py in a fresh process: 16 configurations
    healed first fill heal's table cache, the scrub of a 17th then takes the
    composed path and must still equal locate + heal byte for byte."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = str(tmp_path / "scrub_table_cache.log")
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    cmd = [sys.executable, "-u", os.path.join(root, "tests", "scrub_table_cache_child.py"), "scrub"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT, timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"scrub_table_cache_child.py failed (rc {rc}), {log}:\n{tail}"
    assert "17th configuration scrubbed" in tail, tail
