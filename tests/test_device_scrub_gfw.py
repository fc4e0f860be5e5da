"""leoec_scrub_gfw_dev on the device (product library): locate_gfw and heal in
one call for the GF(2^w) word classes, on the edge harness of gpu_helpers
(guarded arenas, random non-zero bytes behind every object, every byte of both
arenas, the words around the covered ones, the totals' neighbours and the
workspace's tail compared after every call).

The contract is the composition device.locate_gfw then device.heal(lost =
report); the batches are test_device_scrub_ws.py's (scrub_helpers' position
batch, a clean batch, scrub_dev_helpers' dense batch, scrub_helpers'
whole-block batch), for the six word families of locate_gfw_helpers.FAMILIES
with 8,704-byte blocks (two whole 4 KiB tiles and a 512-byte partial one) at
the sizes k B - 1, 16 w (k - 2) + 5 and k B (scrub_dev_helpers.SCRUB_GFW.sizes).
Expected words are by construction (test_scrub_gfw_cpu.py holds them against
the host model).

The position, clean and dense batches damage at most 64 bytes of a block, all
in lane 0's first chunk of one tile: every other byte equals the snapshot
whether gfw_heal_list stored it or not.  The whole-block batch damages every
valid byte of block b in object b: the result is right only if every tile,
every lane, all four chunks, both store paths and the ragged tail were
written.  The dense form of it in a batch of twice the launch's grid runs the
kernel's loop into its second trip in the product library."""
import os
import subprocess
import sys

import pytest

import gpu_helpers as H
import locate_gfw_helpers as G
import locate_helpers as L
import locate_ws_helpers as W
import pending_helpers as PE
import scrub_dev_helpers as D
import scrub_helpers as S
import stream_helpers as T

X, XW = D.SCRUB_GFW, D.SCRUB_WS


@pytest.fixture(scope="module", params=X.FAMILIES, ids=X.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


# every family's block has whole 4 KiB tiles and a last partial one
assert all(B > X.TILE and B % X.TILE != 0 for _, _, _, _, B in X.FAMILIES + [X.LAST])


@pytest.mark.gpu
def test_device_scrub_gfw_positions(gpu, le, oracle, family):
    """One scrub of the position batch: the by-construction report between
    intact sentinels, totals, every named object back to the snapshot, the
    two-block object untouched.  Then the same damage through
    device.locate_gfw + device.heal: identical arenas and words, no object
    left out.  Then a second scrub of the healed arenas: all zero but for the
    two-block object, nothing rebuilt, no byte changed."""
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
        ctx = f"second scrub_gfw {case.ident()} bs {case.bs}"
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
def test_device_scrub_gfw_clean_batch(gpu, le, oracle, family):
    """Nothing damaged: every word 0, totals (0, 0), no byte written."""
    errors = []
    for case in X.cases(le, oracle, family):
        work, par = L.damaged_arenas(gpu, case, [])
        errors += X.check_scrub(gpu, le, case, work, par, [0] * case.n)[1]
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_gfw_dense_batch(gpu, le, oracle, family):
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
def test_device_scrub_gfw_small_workspaces(gpu, le, oracle, family):
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
            ctx = f"scrub_gfw {case.ident()} bs {case.bs} room {room} against one pass"
            work2, par2 = L.damaged_arenas(gpu, case, dmg)
            _, got, tot, errs = X.run_scrub(gpu, le, case, work2, par2, room=room)
            errors += errs
            if got != ref_got or tot != ref_tot:
                errors.append(f"{ctx}: report {[hex(x) for x in got]}, totals {tot}")
            for err in (H.arena_diff(gpu, work2, ref_work, case.guard, f"{ctx}: objs"),
                        H.arena_diff(gpu, par2, ref_par, 1, f"{ctx}: parity")):
                if err:
                    errors.append(err)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_gfw_whole_blocks(gpu, le, oracle, family):
    """Object b has every valid byte of block b damaged: one scrub_gfw, and one
    beside device.locate_gfw + device.heal, both back to the snapshot byte for
    byte; the rebuild was gfw_heal_list's (the list in the workspace).  Then
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


# the smallest block with more than one tile: a full 4 KiB tile and a 256-byte one
LARGE = ("vandrs", 2, 2, 16, 4352)


def test_large_case_is_what_it_says(le, oracle):
    cls, k, m, w, B = LARGE
    assert G.word_class(cls, k, m, w) and B % (16 * w) == 0 and -(-B // X.TILE) == 2
    assert le.layout(cls, (k, m, w), k * B - 1)[0] == B
    assert le.device.scrub_gfw_workspace(cls, (k, m, w), k * B - 1, 1) == 32 + m * B


@pytest.mark.gpu
def test_device_scrub_gfw_batch_larger_than_the_grid(gpu, le, oracle):
    """The dense whole-block batch with objects x tiles at least twice
    gfw_heal_list's grid (compute units x 16 resident workgroups): every
    workgroup takes a second item (`item += gridDim.x`) in the product
    library.  Every object against the oracle's snapshot."""
    cls, k, m, w, B = LARGE
    cus = gpu.cuda.get_device_properties(gpu.cuda.current_device()).multi_processor_count
    tiles = -(-B // X.TILE)
    n = -(-2 * cus * X.resident() // tiles)
    grid = X.grid(cus, n, tiles)
    case = H.EdgeCase(le, oracle, LARGE[:4], k * B - 1, n)
    assert case.bs == B and n * tiles >= 2 * grid and grid == cus * X.resident()
    blocks = S.whole_dense_batch(case)
    want = S.whole_words(case, blocks)
    assert all(x == 1 << (o % (k + m)) for o, x in enumerate(want))  # no object left out
    work, par = S.whole_arenas(gpu, case, blocks)
    keep = []
    errors = X.check_scrub(gpu, le, case, work, par, want, keep=keep)[1]
    assert not errors, "\n".join(e[:2000] for e in errors[:20])
    assert D.path(gpu, keep[0], want) == "list"


@pytest.mark.gpu
def test_device_scrub_gfw_last_id(gpu, le, oracle):
    """vandrs(16,15,8), k + m = 31: every block position, bit 30 the last the
    report can name beside LEOEC_LOCATE_MANY; position and whole-block batches
    at k B - 1."""
    errors = []
    size = X.sizes(X.LAST)[0]
    for case in X.cases(le, oracle, X.LAST, [size]):
        dmg, want, skip = X.position(le, oracle, case)
        assert skip is None and want[30] == 1 << 30 and want[-1] == S.MANY
        work, par = L.damaged_arenas(gpu, case, dmg)
        errors += X.check_scrub(gpu, le, case, work, par, want)[1]
        errors += X.check_equivalence(gpu, le, case, dmg)[4]
    for case in X.whole_cases(le, oracle, X.LAST, [size]):
        path, errs = X.check_whole(gpu, le, case, S.whole_batch(case), composed=False)
        errors += errs
        assert path == "list", path
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [("vandrs", 10, 4, 8, 8704), W.FAMILIES[0]], ids=G.family_id)
def test_device_scrub_gfw_forwards_class_a(gpu, le, oracle, fam):
    """One fused family and one bitmatrix family through device.scrub_gfw equal
    device.scrub_ws: report, totals, arenas, and the workspace size."""
    assert fam in L.FAMILIES or fam in W.FAMILIES
    errors = []
    for case in XW.cases(le, oracle, fam):
        n, g = case.n, case.guard
        dmg, want, skip = XW.position(le, oracle, case)
        assert skip is None
        need = le.device.scrub_ws_workspace(case.cls, case.params, case.size, n)
        assert le.device.scrub_gfw_workspace(case.cls, case.params, case.size, n) == need
        work, par = L.damaged_arenas(gpu, case, dmg)
        work2, par2 = work.clone(), par.clone()
        ws = gpu.full((need + D.WS_TAIL,), D.WS_FILL, dtype=gpu.uint8, device="cuda")
        report, totals = le.device.scrub_gfw(case.cls, case.params, work[g:g + n], case.size,
                                             par[1:1 + n], workspace=ws[:need])
        gpu.cuda.synchronize()
        got, tot = D._u32(report), D._u32(totals)
        _, got2, tot2, errs = XW.run_scrub(gpu, le, case, work2, par2)
        errors += errs
        ctx = f"scrub_gfw against scrub_ws {case.ident()}"
        if (got, tot) != (got2, tot2) or got != want:
            errors.append(f"{ctx}: report {[hex(x) for x in got]} {tot}, scrub_ws's "
                          f"{[hex(x) for x in got2]} {tot2}")
        if not bool((ws[need:] == D.WS_FILL).all()):
            errors.append(f"{ctx}: workspace written past its {need} bytes")
        for err in (H.arena_diff(gpu, work, work2, g, f"{ctx}: objs"),
                    H.arena_diff(gpu, par, par2, 1, f"{ctx}: parity")):
            if err:
                errors.append(err)
    assert not errors, "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# Capture and a side stream (stream_helpers' pattern).

def _stream_case(le, oracle):
    family = X.FAMILIES[0]
    assert family[:4] == ("vandrs", 10, 4, 16)
    return next(iter(X.cases(le, oracle, family)))


@pytest.mark.gpu
def test_device_scrub_gfw_captured(gpu, le, oracle):
    """The call is memsets and launches on the stream: after one plain call
    (the block table, the code objects) it is captured into a graph, writes
    nothing during the capture, and three replays over refilled buffers (the
    position batch, the dense batch, the position batch) give each batch's
    report, totals and arenas."""
    case = _stream_case(le, oracle)
    dmg, want, skip = X.position(le, oracle, case)
    assert skip is None  # m >= 3: every word by construction
    first = L.damaged_arenas(gpu, case, dmg)
    dense, dense_words = D.dense_batch(case)
    second = L.damaged_arenas(gpu, case, dense)
    b = D.Buffers(X, gpu, le, case)
    cap = T.Captured(gpu, b.call, lambda: b.refill(first), lambda: b.untouched(first))
    errors = cap.errors
    for r, (before, words) in enumerate(((first, want), (second, dense_words), (first, want))):
        b.refill(before)
        cap.replay()
        errors += b.check(before, words, f"captured scrub_gfw {case.ident()} replay {r}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_scrub_gfw_on_side_stream(gpu, le, oracle):
    """Behind a large fill and the copies that bring the damaged batch in, on
    a non-blocking side stream, with nothing but that stream's own
    synchronisation afterwards (a plain call on the null stream comes first)."""
    case = _stream_case(le, oracle)
    dmg, want, skip = X.position(le, oracle, case)
    src = L.damaged_arenas(gpu, case, dmg)
    b = D.Buffers(X, gpu, le, case)
    b.refill(src)
    b.call()
    gpu.cuda.synchronize()
    b.refill((gpu.zeros_like(src[0]), gpu.zeros_like(src[1])))
    scratch = gpu.empty((T.WINDOW_BYTES,), dtype=gpu.uint8, device="cuda")
    side = gpu.cuda.Stream()
    assert side.cuda_stream != 0 and side != gpu.cuda.default_stream()
    gpu.cuda.synchronize()  # the buffers above were filled on the null stream
    with gpu.cuda.stream(side):
        scratch.fill_(0x11)
        b.work.copy_(src[0])
        b.par.copy_(src[1])
        b.call(stream=side.cuda_stream)
    side.synchronize()
    errors = b.check(src, want, f"side stream scrub_gfw {case.ident()}")
    assert not errors, "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# A HIP error pending on the calling thread (test_pending_hip_error.py's way:
# hipSetDevice(-1) through the library's own runtime handle, no torch call
# between planting and the clear).

@pytest.mark.gpu
def test_device_scrub_gfw_with_pending_error(gpu, le, oracle):
    """A first plain call, then one with hipErrorInvalidDevice pending on the
    thread: LEOEC_OK, the results right, the same code in the slot afterwards."""
    cls, k, m, w = "vandrs", 6, 3, 32
    B = 4096 + 16 * w
    case = H.edge_case(le, oracle, (cls, k, m, w), k * B - 17, n=3)
    assert case.bs == B
    dmg, want = D.dense_batch(case)
    work, par = L.damaged_arenas(gpu, case, dmg)
    first = X.check_scrub(gpu, le, case, work, par, want)[1]
    assert not first, "\n".join(first)
    dmg = [e for o in range(3) for e in S._entries(case, o, k + o, S.VALUES[:S.HITS])]
    want = [1 << (k + o) for o in range(3)]
    work, par = L.damaged_arenas(gpu, case, dmg)
    calls = []
    with PE.planted(gpu, le, calls, "leoec_scrub_gfw_dev") as rt:
        errors = X.check_scrub(gpu, le, case, work, par, want)[1]
    assert calls == [(0, PE.HIP_ERROR_INVALID_DEVICE)], calls
    assert not errors, "\n".join(errors)
    assert rt.hipPeekAtLastError() == PE.HIP_SUCCESS


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_scrub_gfw_with_full_table_cache_in_own_process(gpu, tmp_path):
    """tests/scrub_table_cache_child.py scrub_gfw in a fresh process: 16 word
    configurations scrubbed first fill the block table cache, the scrub of a
    17th then takes the composed path and must still equal locate_gfw + heal
    byte for byte."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    log = str(tmp_path / "scrub_gfw_table_cache.log")
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    cmd = [sys.executable, "-u", os.path.join(root, "tests", "scrub_table_cache_child.py"), "scrub_gfw"]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT, timeout=280)
    with open(log) as fh:
        tail = fh.read()[-4000:]
    assert rc == 0, f"scrub_table_cache_child.py scrub_gfw failed (rc {rc}), {log}:\n{tail}"
    assert "17th configuration scrubbed" in tail, tail


# ---------------------------------------------------------------------------
# Rows more than 4 GiB apart (wide_helpers' allocation and comparison).

WIDE = ("vandrs", 10, 4, 16, 8704)


def _wide_plan(le, oracle, variant):
    """wide_helpers.plan_scrub for device.scrub_gfw: the whole-block damage of
    wide_helpers.locate_blocks, the words by construction (and the host
    model's), the named blocks back to the oracle's bytes."""
    import wide_helpers as Wd
    assert WIDE in Wd.FAMILIES
    case, lay = Wd.wide_case(le, oracle, WIDE), Wd.layout(le, WIDE)
    blocks = Wd.locate_blocks(case)
    p = Wd.Plan(case, lay, "scrub_gfw", variant)
    p.want = Wd._base(lay, case)
    p.pre = Wd._copy(p.want)
    p.outputs = Wd._damage(lay, case, p.pre, blocks)
    want = S.whole_words(case, blocks)
    assert G.words_of(oracle, le, case, S.whole_objects(case, blocks)) == want
    assert D.counts(want) == [2, 0]
    p.words_pre = {"report": Wd._sentinels([L.PREFILL] * Wd.NOBJ, L.SENTINELS),
                   "totals": Wd._sentinels([D.TOTALS_PREFILL] * 2, L.SENTINELS)}
    p.words_want = {"report": Wd._sentinels(want, L.SENTINELS),
                    "totals": Wd._sentinels(D.counts(want), L.SENTINELS),
                    "workspace tail": Wd.WS_TAIL_WANT}
    need = X.workspace_bytes(le, case, 1 if variant == "min" else None)

    def run(gpu, le, arena, words):
        objs, par = Wd._views(arena, lay, case)
        report, totals = Wd._i32(gpu, words["report"]), Wd._i32(gpu, words["totals"])
        ws = Wd._workspace(gpu, need)
        le.device.scrub_gfw(case.cls, case.params, objs, case.size, par, report=report[1:1 + Wd.NOBJ],
                            totals=totals[1:3], workspace=ws[:need])
        gpu.cuda.synchronize()
        p.info["path"] = D.path(gpu, ws, want[-1:] if variant == "min" else want)
        return {"report": D._u32(report), "totals": D._u32(totals), "workspace tail": Wd._tail(ws, need)}
    p.run = run
    return p


@pytest.mark.gpu
def test_device_scrub_gfw_wide_strides(gpu, le, oracle):
    """Three objects whose rows lie 2^32 + 48 bytes apart, with the query's
    workspace and with room for one object (the chunk loop's host-side
    o0 * stride)."""
    import wide_helpers as Wd
    try:
        arena = Wd.Arena(gpu, Wd.arena_used(le))
    except RuntimeError as e:  # (torch's out-of-memory error is one)
        pytest.skip(f"the wide allocation cannot be made: {str(e)[:200]}")
    try:
        errors = []
        for variant in ("query", "min"):
            p = _wide_plan(le, oracle, variant)
            errors += Wd.execute(gpu, le, arena, p)
            if p.info.get("path") != "list":
                errors.append(f"{p.ident()}: not the kernel path: {p.info.get('path')}")
    finally:
        arena.release()
    assert not errors, "\n".join(errors[:12])
