"""Shared pieces of the leoec_scrub_gfw_dev tests (test_scrub_gfw_cpu.py, no
GPU; test_device_scrub_gfw.py, test_scrub_gfw_forms.py and
scrub_gfw_table_cache_child.py on the device): scrub_ws_helpers' run_scrub,
check_scrub, check_equivalence and check_whole for device.scrub_gfw and the
two-call sequence device.locate_gfw + device.heal the call must equal byte for
byte.  The batches are scrub_helpers' and scrub_dev_helpers', unchanged; the
families locate_gfw_helpers.FAMILIES; the word the two-block object of an m = 2
family gets is locate_gfw_helpers' host model's."""
import gpu_helpers as H
import locate_gfw_helpers as G
import locate_helpers as L
import scrub_dev_helpers as D
import scrub_helpers as S

MANY = L.MANY
WS_FILL, WS_TAIL, TOTALS_PREFILL = D.WS_FILL, D.WS_TAIL, D.TOTALS_PREFILL
_hex, _u32 = D._hex, D._u32
TILE = 4096  # bytes of a block one workgroup of gfw_heal_list takes per item (gfw_heal_tile.hpp)
FAMILIES = G.FAMILIES
LAST = ("vandrs", 16, 15, 8, 8704)  # k + m = 31: the last id the report has a bit for


def sizes(family):
    """k B - 1 (the last data block one byte short: whole tiles take the
    kernel's unguarded stores, the last, partial tile the guarded ones),
    16 w (k - 2) + 5 (one partial tile; data block k - 2 holds 5 valid bytes, a
    w = 16 / 32 word cut in the middle, block k - 1 is empty) and k B (no block
    clipped)."""
    cls, k, m, w, B = family
    out = D.sizes(family) + [k * B]
    assert out == [k * B - 1, 16 * w * (k - 2) + 5, k * B]
    return out


def cases(le, oracle, family, sizes_=None):
    """The k + m + 2 objects of scrub_helpers' position batch at every size."""
    cls, k, m, w, B = family
    for size in sizes_ or sizes(family):
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 2)


def whole_cases(le, oracle, family, sizes_=None):
    """The k + m + 1 objects of scrub_helpers' whole-block batch at every size."""
    cls, k, m, w, B = family
    for size in sizes_ or sizes(family):
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 1)


def position(le, oracle, case):
    """(damage list, by-construction report, skip) of the position batch: where
    scrub_helpers.position_batch leaves the two-block object's word open
    (m = 2: LEOEC_LOCATE_MANY or a third block, the documented limit) it is
    the host model's, and the object is left out of the byte comparison when
    that names a block."""
    dmg, _, locate = S.position_batch(case)
    want = list(locate)
    two = case.n - 1
    if want[two] is None:
        word = G.words_of(oracle, le, case, S.damaged_objects(case, dmg, [two]))[two]
        k, m = case.k, case.m
        assert word == MANY or (word in [1 << b for b in range(k + m)]
                                and word not in (1, 1 << (k + m - 1))), (case.ident(), hex(word))
        want[two] = word
    skip = None if want[two] == MANY else two
    assert skip is None or case.m == 2
    return dmg, want, skip


def head(nobj):
    """The header and the index words."""
    return 16 + (4 * nobj + 15) // 16 * 16


def workspace_bytes(le, case, room=None):
    """The query's size (one pass), or the header, the index words and an
    encode region for `room` objects (1: the minimum)."""
    n = case.n
    need = le.device.scrub_gfw_workspace(case.cls, case.params, case.size, n)
    assert need == head(n) + n * case.m * case.bs
    return need if room is None else head(n) + room * case.m * case.bs


def run_scrub(gpu, le, case, work, par, room=None, keep=None):
    """One device.scrub_gfw: report in a pre-filled [n + 2] tensor (words 1..n
    covered), totals in a [4] tensor (words 1..2), the workspace in WS_FILL
    bytes with WS_TAIL more behind its size.  Returns (the [n + 2] report
    tensor, its n covered words, the two totals, errors): the sentinel words
    and the workspace's tail intact.  `keep`: a list the workspace tensor is
    appended to, as the call leaves it (scrub_dev_helpers.path)."""
    n, g = case.n, case.guard
    report = gpu.full((n + 2,), L.PREFILL, dtype=gpu.int32, device="cuda")
    report[0], report[n + 1] = L.SENTINELS
    totals = gpu.full((4,), TOTALS_PREFILL, dtype=gpu.int32, device="cuda")
    totals[0], totals[3] = L.SENTINELS
    need = workspace_bytes(le, case, room)
    ws = gpu.full((need + WS_TAIL,), WS_FILL, dtype=gpu.uint8, device="cuda")
    out = le.device.scrub_gfw(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                              report=report[1:1 + n], totals=totals[1:3], workspace=ws[:need])
    gpu.cuda.synchronize()
    assert out[0].data_ptr() == report[1:1 + n].data_ptr() and out[1].data_ptr() == totals[1:3].data_ptr()
    got, tot = _u32(report), _u32(totals)
    ctx = f"scrub_gfw {case.ident()} bs {case.bs} room {room}"
    errors = []
    if (got[0], got[-1]) != L.SENTINELS:
        errors.append(f"{ctx}: report sentinels {got[0]:#x}, {got[-1]:#x}")
    if (tot[0], tot[3]) != L.SENTINELS:
        errors.append(f"{ctx}: totals sentinels {tot[0]:#x}, {tot[3]:#x}")
    if not bool((ws[need:] == WS_FILL).all()):
        errors.append(f"{ctx}: workspace written past its {need} bytes")
    if keep is not None:
        keep.append(ws)
    return report, got[1:-1], tot[1:3], errors


def counts(words):
    return [sum(1 for x in words if x not in (0, MANY)), sum(1 for x in words if x == MANY)]


def check_scrub(gpu, le, case, work, par, want, skip=None, room=None, keep=None):
    """run_scrub against the by-construction words: report == want, totals ==
    (single-bit words, MANY words), every object whose word names a block back
    to the snapshot byte for byte, a MANY object as it was damaged, guard rows
    and bytes past `size` unchanged.  `skip`: an object whose word and bytes
    are not compared.  Returns (the [n + 2] report tensor, the errors)."""
    n, g = case.n, case.guard
    snap, par_snap = case.dev(gpu)
    before, par_before = work.clone(), par.clone()
    report, got, tot, errors = run_scrub(gpu, le, case, work, par, room, keep)
    ctx = f"scrub_gfw {case.ident()} bs {case.bs} room {room}"
    expect = list(want)
    if skip is not None:
        expect[skip] = got[skip]
    if got != expect:
        bad = [o for o in range(n) if got[o] != expect[o]]
        errors.append(f"{ctx}: objects {bad}: report {_hex(got)}, expected {_hex(expect)}")
    if tot != counts(expect):
        errors.append(f"{ctx}: totals {tot}, expected {counts(expect)}")
    objs_want, par_want = snap.clone(), par_snap.clone()
    for o, word in enumerate(expect):
        if word == MANY:
            objs_want[g + o], par_want[1 + o] = before[g + o], par_before[1 + o]
    if skip is not None:
        objs_want[g + skip], par_want[1 + skip] = work[g + skip], par[1 + skip]
    for err in (H.arena_diff(gpu, work, objs_want, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par_want, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return report, errors


def locate_then_heal(gpu, le, case, work, par):
    """device.locate_gfw then device.heal with its words, in place; the words."""
    n, g = case.n, case.guard
    lost = le.device.locate_gfw(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n])
    le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], lost)
    gpu.cuda.synchronize()
    return _u32(lost)


def check_equivalence(gpu, le, case, dmg, room=None, arenas=None):
    """The damaged arenas twice: one through device.scrub_gfw, one through
    device.locate_gfw + device.heal.  Both arenas byte for byte and lost ==
    report, no object left out.  Returns (scrub_gfw's arenas, its report
    words, its totals, errors)."""
    g = case.guard
    work, par = L.damaged_arenas(gpu, case, dmg) if dmg is not None else arenas
    work2, par2 = work.clone(), par.clone()
    _, got, tot, errors = run_scrub(gpu, le, case, work, par, room)
    lost = locate_then_heal(gpu, le, case, work2, par2)
    ctx = f"scrub_gfw against locate_gfw + heal {case.ident()} bs {case.bs} room {room}"
    if lost != got:
        errors.append(f"{ctx}: report {_hex(got)}, lost {_hex(lost)}")
    for err in (H.arena_diff(gpu, work, work2, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par2, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return work, par, got, tot, errors


def check_whole(gpu, le, case, blocks, room=None, composed=True):
    """scrub_helpers' whole-block damage of `blocks` through one call (the
    by-construction report and totals, every byte back to the snapshot) and,
    with `composed`, once more beside device.locate_gfw + device.heal, whose
    arenas are compared with the snapshot as well.  Returns (the first call's
    path, the errors)."""
    want = S.whole_words(case, blocks)
    keep = []
    work, par = S.whole_arenas(gpu, case, blocks)
    errors = ["whole blocks: " + e
              for e in check_scrub(gpu, le, case, work, par, want, room=room, keep=keep)[1]]
    if composed:
        work, par, got, _, errs = check_equivalence(gpu, le, case, None, room,
                                                    S.whole_arenas(gpu, case, blocks))
        errors += ["whole blocks: " + e for e in errs]
        snap, par_snap = case.dev(gpu)
        ctx = f"whole blocks: scrub_gfw beside locate_gfw + heal {case.ident()} bs {case.bs} room {room}"
        if got != want:
            errors.append(f"{ctx}: report {_hex(got)}, expected {_hex(want)}")
        for err in (H.arena_diff(gpu, work, snap, case.guard, f"{ctx}: objs"),
                    H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity")):
            if err:
                errors.append(err)
    return D.path(gpu, keep[0], want), errors


def gfw_heal_list_resident():
    """gfw_heal_list_resident() of gfw_heal_tile.hpp, restated: one wave per
    workgroup, 4 waves on each of a compute unit's 4 SIMDs."""
    return 16


def grid(cus, nobj, tiles, cap=0):
    """launch_gfw_heal_list's grid (list_grid, heal_impl.hpp), restated."""
    g = min(cus * gfw_heal_list_resident(), nobj * tiles)
    return min(g, cap) if cap else g
