"""Shared pieces of the leoec_scrub_dev tests (test_device_scrub.py,
test_scrub_forms.py, scrub_table_cache_child.py): one device.scrub over
arenas the caller damaged, with everything the call may not touch compared
afterwards, the expectations of scrub_helpers' position batch and of the dense
batch, the two-call sequence device.locate + device.heal the call must equal
byte for byte, scrub_helpers' whole-block batch through both, and which path a
call took, read from the workspace it leaves."""
import gpu_helpers as H
import locate_helpers as L
import scrub_helpers as S

MANY = L.MANY
WS_FILL = 0x6B   # every workspace byte before the call
WS_TAIL = 64     # bytes allocated past the query's size: never written
TOTALS_PREFILL = 0x707A15


def _hex(words):
    return [hex(x) for x in words]


def _u32(t):
    return [int(x) & 0xFFFFFFFF for x in t.cpu().tolist()]


def sizes(family):
    """test_device_scrub_positions.py's two sizes: k B - 1 and 16 w (k - 2) + 5."""
    cls, k, m, w, B = family
    out = [k * B - 1, 16 * w * (k - 2) + 5]
    assert all(s in H.edge_sizes(k, w, B) for s in out)
    return out


def position_cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in sizes(family):
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 2)


def whole_cases(le, oracle, family):
    """position_cases' sizes with the k + m + 1 objects of scrub_helpers'
    whole-block batch."""
    cls, k, m, w, B = family
    for size in sizes(family):
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 1)


def dense_batch(case):
    """(damage list, locate words): object o has block o mod (k + m) damaged
    (scrub_helpers' 64 values at block_hits' places); a data block wholly past
    `size` has no byte to damage and its object expects 0."""
    dmg, words = [], []
    for o in range(case.n):
        b = o % (case.k + case.m)
        hits = S._entries(case, o, b, S.VALUES[:S.HITS])
        dmg += hits
        words.append(1 << b if hits else 0)
    return dmg, words


def run_scrub(gpu, le, case, work, par, buffers=None, keep=None):
    """One device.scrub over the given arenas.  report lies in a pre-filled
    [n + 2] tensor (words 1..n covered), totals in a [4] tensor (words 1..2),
    the workspace in WS_FILL bytes with WS_TAIL more behind the query's size.
    Returns (the [n + 2] report tensor, its n covered words, the two totals,
    errors): the sentinel words and the workspace's tail intact.  `keep`: a
    list the workspace tensor is appended to, as the call leaves it (path)."""
    n, g = case.n, case.guard
    report = gpu.full((n + 2,), L.PREFILL, dtype=gpu.int32, device="cuda")
    report[0], report[n + 1] = L.SENTINELS
    totals = gpu.full((4,), TOTALS_PREFILL, dtype=gpu.int32, device="cuda")
    totals[0], totals[3] = L.SENTINELS
    need = le.device.scrub_workspace(case.cls, case.params, case.size, n)
    assert need == 16 + (4 * n + 15) // 16 * 16
    ws = gpu.full((need + WS_TAIL,), WS_FILL, dtype=gpu.uint8, device="cuda")
    out = le.device.scrub(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                          report=report[1:1 + n], totals=totals[1:3], workspace=ws[:need])
    gpu.cuda.synchronize()
    assert out[0].data_ptr() == report[1:1 + n].data_ptr() and out[1].data_ptr() == totals[1:3].data_ptr()
    got, tot = _u32(report), _u32(totals)
    ctx = f"scrub {case.ident()} bs {case.bs}"
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


def path(gpu, ws, words):
    """Which path a call took, from the workspace it leaves (scrub.hip): "list"
    when header word 0 is the number of objects whose word in `words` (the
    report, or what it must be) names a block and the index words before it
    are a permutation of those objects
    (scrub_finish's list, which only the rebuild kernel reads), "composed" when
    the header is as it was filled and the index words are leoec_heal_dev's
    `unhealed`, anything else as a description."""
    n = len(words)
    left = _u32(ws[:16 + 4 * n].view(gpu.int32))
    count, index = left[0], left[4:4 + n]
    named = [o for o, x in enumerate(words) if x not in (0, MANY)]
    if count == len(named) and sorted(index[:count]) == named:
        return "list"
    if count == int.from_bytes(bytes([WS_FILL]) * 4, "little"):
        return "composed"
    return f"header word {count:#x}, index words {index[:16]}"


def check_scrub(gpu, le, case, work, par, want, skip=None, keep=None):
    """run_scrub of arenas damaged from the case's snapshots, against the
    by-construction words `want`: report == want, totals == (single-bit words,
    MANY words), every object whose word names a block back to the snapshot
    byte for byte, a MANY object as it was damaged, guard rows and bytes past
    `size` unchanged.  `skip`: an object whose word and bytes are not compared
    (m = 2: two damaged blocks explained by a third); it counts as whatever
    its word says.  Returns (the [n + 2] report tensor, the errors)."""
    n, g = case.n, case.guard
    snap, par_snap = case.dev(gpu)
    before, par_before = work.clone(), par.clone()
    report, got, tot, errors = run_scrub(gpu, le, case, work, par, keep=keep)
    ctx = f"scrub {case.ident()} bs {case.bs}"
    expect = list(want)
    if skip is not None:
        expect[skip] = got[skip]
    if got != expect:
        bad = [o for o in range(n) if got[o] != expect[o]]
        errors.append(f"{ctx}: objects {bad}: report {_hex(got)}, expected {_hex(expect)}")
    counts = [sum(1 for x in expect if x not in (0, MANY)), sum(1 for x in expect if x == MANY)]
    if tot != counts:
        errors.append(f"{ctx}: totals {tot}, expected {counts}")
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
    """device.locate then device.heal with its words, in place; the words."""
    n, g = case.n, case.guard
    lost = le.device.locate(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n])
    le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], lost)
    gpu.cuda.synchronize()
    return _u32(lost)


def check_equivalence(gpu, le, case, dmg, arenas=None):
    """The damaged arenas twice: one through device.scrub, one through
    device.locate + device.heal.  Both arenas byte for byte and lost == report,
    no object left out.  The arenas are damaged_arenas' of the list `dmg`, or
    (dmg None) the pair `arenas`, damaged by the caller and taken over.
    Returns (scrub's arenas, its report words, errors)."""
    n, g = case.n, case.guard
    work, par = L.damaged_arenas(gpu, case, dmg) if dmg is not None else arenas
    work2, par2 = work.clone(), par.clone()
    _, got, tot, errors = run_scrub(gpu, le, case, work, par)
    lost = locate_then_heal(gpu, le, case, work2, par2)
    ctx = f"scrub against locate + heal {case.ident()} bs {case.bs}"
    if lost != got:
        errors.append(f"{ctx}: report {_hex(got)}, lost {_hex(lost)}")
    for err in (H.arena_diff(gpu, work, work2, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par2, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return work, par, got, errors


def check_whole(gpu, le, case, blocks):
    """scrub_helpers' whole-block damage of `blocks` through one device.scrub
    (check_scrub: the by-construction report and totals, every byte back to
    the snapshot) and once more beside device.locate + device.heal
    (check_equivalence), whose arenas are compared with the snapshot as well.
    Returns (the first call's path, the errors)."""
    want = S.whole_words(case, blocks)
    keep = []
    work, par = S.whole_arenas(gpu, case, blocks)
    errors = ["whole blocks: " + e for e in check_scrub(gpu, le, case, work, par, want, keep=keep)[1]]
    work, par, got, errs = check_equivalence(gpu, le, case, None, S.whole_arenas(gpu, case, blocks))
    errors += ["whole blocks: " + e for e in errs]
    snap, par_snap = case.dev(gpu)
    ctx = f"whole blocks: scrub beside locate + heal {case.ident()} bs {case.bs}"
    if got != want:
        errors.append(f"{ctx}: report {_hex(got)}, expected {_hex(want)}")
    for err in (H.arena_diff(gpu, work, snap, case.guard, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return path(gpu, keep[0], want), errors
