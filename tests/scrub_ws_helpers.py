"""Shared pieces of the leoec_scrub_ws_dev tests (test_device_scrub_ws.py,
test_scrub_ws_forms.py, scrub_ws_table_cache_child.py): scrub_dev_helpers'
run_scrub, check_scrub and check_equivalence for device.scrub_ws and the
two-call sequence device.locate_ws + device.heal the call must equal byte for
byte.  The batches and their expected words are scrub_helpers' and
scrub_dev_helpers', unchanged."""
import gpu_helpers as H
import locate_helpers as L
import scrub_dev_helpers as D
import scrub_helpers as S

MANY = L.MANY
WS_FILL, WS_TAIL, TOTALS_PREFILL = D.WS_FILL, D.WS_TAIL, D.TOTALS_PREFILL
_hex, _u32 = D._hex, D._u32
TILE = 1024  # bytes of a packet one workgroup of bit_heal_list takes (bit_heal_tile.hpp)


def cases(le, oracle, family):
    """scrub_dev_helpers.position_cases' two sizes (k B - 1: the last data
    block one byte short, so the whole tiles of a packet take the kernel's
    unguarded loads and stores and every packet's last, partial tile the
    guarded ones; 16 w (k - 2) + 5: one partial tile, an empty and a ragged
    data block), then k B: no block clipped at all, the shape of an object
    whose size is a multiple of 16 k w."""
    cls, k, m, w, B = family
    yield from D.position_cases(le, oracle, family)
    assert k * B in H.edge_sizes(k, w, B)
    yield H.edge_case(le, oracle, family[:4], k * B, n=k + m + 2)


def whole_cases(le, oracle, family):
    """cases' three sizes with the k + m + 1 objects of scrub_helpers'
    whole-block batch."""
    cls, k, m, w, B = family
    for size in D.sizes(family) + [k * B]:
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 1)


def head(nobj):
    """The header and the index words."""
    return 16 + (4 * nobj + 15) // 16 * 16


def workspace_bytes(le, case, room=None):
    """The query's size (one pass), or the header, the index words and an
    encode region for `room` objects (bitmatrix classes; 1: the minimum)."""
    n = case.n
    need = le.device.scrub_ws_workspace(case.cls, case.params, case.size, n)
    if case.cls in ("cauchyrs", "liberation"):
        assert need == head(n) + n * case.m * case.bs
        if room is not None:
            need = head(n) + room * case.m * case.bs
    else:
        assert need == head(n) == le.device.scrub_workspace(case.cls, case.params, case.size, n)
    return need


def run_scrub(gpu, le, case, work, par, room=None, keep=None):
    """scrub_dev_helpers.run_scrub for device.scrub_ws: report in a pre-filled
    [n + 2] tensor (words 1..n covered), totals in a [4] tensor (words 1..2),
    the workspace in WS_FILL bytes with WS_TAIL more behind its size.  Returns
    (the [n + 2] report tensor, its n covered words, the two totals, errors):
    the sentinel words and the workspace's tail intact.  `keep`: a list the
    workspace tensor is appended to, as the call leaves it
    (scrub_dev_helpers.path; with room for fewer objects than the batch the
    header and the list are the last chunk's)."""
    n, g = case.n, case.guard
    report = gpu.full((n + 2,), L.PREFILL, dtype=gpu.int32, device="cuda")
    report[0], report[n + 1] = L.SENTINELS
    totals = gpu.full((4,), TOTALS_PREFILL, dtype=gpu.int32, device="cuda")
    totals[0], totals[3] = L.SENTINELS
    need = workspace_bytes(le, case, room)
    ws = gpu.full((need + WS_TAIL,), WS_FILL, dtype=gpu.uint8, device="cuda")
    out = le.device.scrub_ws(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                             report=report[1:1 + n], totals=totals[1:3], workspace=ws[:need])
    gpu.cuda.synchronize()
    assert out[0].data_ptr() == report[1:1 + n].data_ptr() and out[1].data_ptr() == totals[1:3].data_ptr()
    got, tot = _u32(report), _u32(totals)
    ctx = f"scrub_ws {case.ident()} bs {case.bs} room {room}"
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


def check_scrub(gpu, le, case, work, par, want, skip=None, room=None, keep=None):
    """scrub_dev_helpers.check_scrub for device.scrub_ws: report == want,
    totals == (single-bit words, MANY words), every object whose word names a
    block back to the snapshot byte for byte, a MANY object as it was damaged,
    guard rows and bytes past `size` unchanged.  `skip`: an object whose word
    and bytes are not compared (m = 2: two damaged blocks explained by a
    third).  Returns (the [n + 2] report tensor, the errors)."""
    n, g = case.n, case.guard
    snap, par_snap = case.dev(gpu)
    before, par_before = work.clone(), par.clone()
    report, got, tot, errors = run_scrub(gpu, le, case, work, par, room, keep)
    ctx = f"scrub_ws {case.ident()} bs {case.bs} room {room}"
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
    """device.locate_ws then device.heal with its words, in place; the words."""
    n, g = case.n, case.guard
    lost = le.device.locate_ws(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n])
    le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], lost)
    gpu.cuda.synchronize()
    return _u32(lost)


def check_equivalence(gpu, le, case, dmg, room=None, arenas=None):
    """The damaged arenas twice: one through device.scrub_ws, one through
    device.locate_ws + device.heal.  Both arenas byte for byte and lost ==
    report, no object left out.  The arenas are damaged_arenas' of the list
    `dmg`, or (dmg None) the pair `arenas`, damaged by the caller and taken
    over.  Returns (scrub_ws's arenas, its report words, its totals, errors)."""
    g = case.guard
    work, par = L.damaged_arenas(gpu, case, dmg) if dmg is not None else arenas
    work2, par2 = work.clone(), par.clone()
    _, got, tot, errors = run_scrub(gpu, le, case, work, par, room)
    lost = locate_then_heal(gpu, le, case, work2, par2)
    ctx = f"scrub_ws against locate_ws + heal {case.ident()} bs {case.bs} room {room}"
    if lost != got:
        errors.append(f"{ctx}: report {_hex(got)}, lost {_hex(lost)}")
    for err in (H.arena_diff(gpu, work, work2, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par2, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return work, par, got, tot, errors


def check_whole(gpu, le, case, blocks, room=None):
    """scrub_dev_helpers.check_whole for device.scrub_ws: scrub_helpers'
    whole-block damage of `blocks` through one call (the by-construction report
    and totals, every byte back to the snapshot) and once more beside
    device.locate_ws + device.heal, whose arenas are compared with the snapshot
    as well.  Returns (the first call's path, the errors)."""
    want = S.whole_words(case, blocks)
    keep = []
    work, par = S.whole_arenas(gpu, case, blocks)
    errors = ["whole blocks: " + e
              for e in check_scrub(gpu, le, case, work, par, want, room=room, keep=keep)[1]]
    work, par, got, _, errs = check_equivalence(gpu, le, case, None, room, S.whole_arenas(gpu, case, blocks))
    errors += ["whole blocks: " + e for e in errs]
    snap, par_snap = case.dev(gpu)
    ctx = f"whole blocks: scrub_ws beside locate_ws + heal {case.ident()} bs {case.bs} room {room}"
    if got != want:
        errors.append(f"{ctx}: report {_hex(got)}, expected {_hex(want)}")
    for err in (H.arena_diff(gpu, work, snap, case.guard, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return D.path(gpu, keep[0], want), errors
