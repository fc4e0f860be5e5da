"""The one harness of the leoec_scrub_dev, leoec_scrub_ws_dev and
leoec_scrub_gfw_dev tests (test_device_scrub*.py, test_scrub*_forms.py,
test_scrub_ws_cpu.py, test_scrub_gfw_cpu.py, test_scrub_whole_cpu.py,
test_pending_hip_error.py, wide_helpers.py, scrub_table_cache_child.py and the
scrub*_instances_child.py scripts).  A `Call` describes what differs between
the three calls (SCRUB, SCRUB_WS, SCRUB_GFW); its methods are the harness: one
call over arenas the caller damaged, with everything the call may not touch
compared afterwards, the expectations of scrub_helpers' position batch and of
the dense batch, the two-call sequence locate + device.heal the call must equal
byte for byte, scrub_helpers' whole-block batch through both, and which path a
call took, read from the workspace it leaves."""
import gpu_helpers as H
import locate_gfw_helpers as G
import locate_helpers as L
import locate_ws_helpers as W
import scrub_helpers as S
import stream_helpers as T

MANY = L.MANY
WS_FILL = 0x6B   # every workspace byte before the call
WS_TAIL = 64     # bytes allocated past the workspace's size: never written
TOTALS_PREFILL = 0x707A15


def _hex(words):
    return [hex(x) for x in words]


def _u32(t):
    return [int(x) & 0xFFFFFFFF for x in t.cpu().tolist()]


def head(nobj):
    """The header and the index words."""
    return 16 + (4 * nobj + 15) // 16 * 16


def counts(words):
    """The totals of a report: (single-bit words, MANY words)."""
    return [sum(1 for x in words if x not in (0, MANY)), sum(1 for x in words if x == MANY)]


def sizes(family):
    """test_device_scrub_positions.py's two sizes: k B - 1 (the last data block
    one byte short: whole tiles take the kernels' unguarded loads and stores,
    the last, partial tile the guarded ones) and 16 w (k - 2) + 5 (one partial
    tile; data block k - 2 holds 5 valid bytes, a w = 16 / 32 word cut in the
    middle, block k - 1 is empty)."""
    cls, k, m, w, B = family
    out = [k * B - 1, 16 * w * (k - 2) + 5]
    assert all(s in H.edge_sizes(k, w, B) for s in out)
    return out


def sizes_and_whole(family):
    """sizes, then k B: no block clipped at all, the shape of an object whose
    size is a multiple of 16 k w."""
    cls, k, m, w, B = family
    assert k * B in H.edge_sizes(k, w, B)
    return sizes(family) + [k * B]


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


def path(gpu, ws, words):
    """Which path a call took, from the workspace it leaves (scrub.hip): "list"
    when header word 0 is the number of objects whose word in `words` (the
    report, or what it must be) names a block and the index words before it
    are a permutation of those objects
    (scrub_finish's list, which only the rebuild kernel reads), "composed" when
    the header is as it was filled and the index words are leoec_heal_dev's
    `unhealed`, anything else as a description.  (With room for fewer objects
    than the batch the header and the list are the last chunk's.)"""
    n = len(words)
    left = _u32(ws[:16 + 4 * n].view(gpu.int32))
    count, index = left[0], left[4:4 + n]
    named = [o for o, x in enumerate(words) if x not in (0, MANY)]
    if count == len(named) and sorted(index[:count]) == named:
        return "list"
    if count == int.from_bytes(bytes([WS_FILL]) * 4, "little"):
        return "composed"
    return f"header word {count:#x}, index words {index[:16]}"


class Call:
    """One of device.scrub, device.scrub_ws and device.scrub_gfw:

    name           the device function; name + "_workspace" its query
    locate         the device function of the two-call sequence
    encode_region  the classes the call does not forward to device.scrub keep
                   an encode region behind the header, which `room` can shrink
    FAMILIES, family_id   the call's own families (the product tests' fixture)
    LAST           scrub_gfw: k + m = 31, the last id the report has a bit for
    sizes          the sizes of cases() and whole_cases()
    words_of       the host model of the two-block object's word at m = 2
    TILE           bytes one workgroup of the call's list kernel takes per item
    resident       workgroups of that kernel resident on a compute unit, restated
    """

    def __init__(self, name, locate, encode_region, families, family_id, last, sizes, words_of, tile,
                 resident):
        self.name, self.locate, self.encode_region = name, locate, encode_region
        self.FAMILIES, self.family_id, self.LAST = families, family_id, last
        self.sizes, self.words_of, self.TILE, self.resident = sizes, words_of, tile, resident

    def grid(self, cus, nobj, tiles, cap=0, *shape):
        """The list kernel's grid (list_grid, heal_impl.hpp), restated; `shape`
        is what resident() takes."""
        g = min(cus * self.resident(*shape), nobj * tiles)
        return min(g, cap) if cap else g

    def cases(self, le, oracle, family, sizes_=None):
        """The k + m + 2 objects of scrub_helpers' position batch at every size."""
        cls, k, m, w, B = family
        for size in sizes_ or self.sizes(family):
            yield H.edge_case(le, oracle, family[:4], size, n=k + m + 2)

    def whole_cases(self, le, oracle, family, sizes_=None):
        """The k + m + 1 objects of scrub_helpers' whole-block batch at every size."""
        cls, k, m, w, B = family
        for size in sizes_ or self.sizes(family):
            yield H.edge_case(le, oracle, family[:4], size, n=k + m + 1)

    def position(self, le, oracle, case):
        """(damage list, by-construction report, skip) of the position batch:
        where scrub_helpers.position_batch leaves the two-block object's word
        open (m = 2: LEOEC_LOCATE_MANY or a third block, the documented limit)
        it is the host model's, and the object is left out of the byte
        comparison when that names a block."""
        dmg, _, locate = S.position_batch(case)
        want = list(locate)
        two = case.n - 1
        if want[two] is None:
            word = self.words_of(oracle, le, case, S.damaged_objects(case, dmg, [two]))[two]
            k, m = case.k, case.m
            assert word == MANY or (word in [1 << b for b in range(k + m)]
                                    and word not in (1, 1 << (k + m - 1))), (case.ident(), hex(word))
            want[two] = word
        skip = None if want[two] == MANY else two
        assert skip is None or case.m == 2
        return dmg, want, skip

    def workspace_bytes(self, le, case, room=None):
        """The query's size (one pass), or, where the call keeps an encode
        region for the case's class, the header, the index words and an encode
        region for `room` objects (1: the minimum).  What the call forwards to
        device.scrub needs device.scrub's bytes."""
        n = case.n
        need = getattr(le.device, self.name + "_workspace")(case.cls, case.params, case.size, n)
        if self.encode_region and not L.served(case.cls, *case.params):
            assert need == head(n) + n * case.m * case.bs
            if room is not None:
                need = head(n) + room * case.m * case.bs
        else:
            assert need == head(n) == le.device.scrub_workspace(case.cls, case.params, case.size, n)
        return need

    def ctx(self, case, room=None, what=None):
        """The head of an error line: what ran (the call), the case, the room."""
        return (f"{what or self.name} {case.ident()} bs {case.bs}"
                + (f" room {room}" if self.encode_region else ""))

    def run_scrub(self, gpu, le, case, work, par, room=None, keep=None):
        """One call over the given arenas.  report lies in a pre-filled [n + 2]
        tensor (words 1..n covered), totals in a [4] tensor (words 1..2), the
        workspace in WS_FILL bytes with WS_TAIL more behind its size
        (workspace_bytes).  Returns (the [n + 2] report tensor, its n covered
        words, the two totals, errors): the sentinel words and the workspace's
        tail intact.  `keep`: a list the workspace tensor is appended to, as
        the call leaves it (path)."""
        b = Buffers(self, gpu, le, case, room, arenas=(work, par))
        out = b.call()
        gpu.cuda.synchronize()
        n = case.n
        assert (out[0].data_ptr() == b.report[1:1 + n].data_ptr()
                and out[1].data_ptr() == b.totals[1:3].data_ptr())
        got, tot = _u32(b.report), _u32(b.totals)
        ctx = self.ctx(case, room)
        errors = []
        if (got[0], got[-1]) != L.SENTINELS:
            errors.append(f"{ctx}: report sentinels {got[0]:#x}, {got[-1]:#x}")
        if (tot[0], tot[3]) != L.SENTINELS:
            errors.append(f"{ctx}: totals sentinels {tot[0]:#x}, {tot[3]:#x}")
        errors += b.tail_errors(ctx)
        if keep is not None:
            keep.append(b.ws)
        return b.report, got[1:-1], tot[1:3], errors

    def check_scrub(self, gpu, le, case, work, par, want, skip=None, room=None, keep=None):
        """run_scrub of arenas damaged from the case's snapshots, against the
        by-construction words `want`: report == want, totals == (single-bit
        words, MANY words), every object whose word names a block back to the
        snapshot byte for byte, a MANY object as it was damaged, guard rows and
        bytes past `size` unchanged.  `skip`: an object whose word and bytes
        are not compared (m = 2: two damaged blocks explained by a third); it
        counts as whatever its word says.  Returns (the [n + 2] report tensor,
        the errors)."""
        n, g = case.n, case.guard
        before = (work.clone(), par.clone())
        report, got, tot, errors = self.run_scrub(gpu, le, case, work, par, room, keep)
        ctx = self.ctx(case, room)
        expect = list(want)
        if skip is not None:
            expect[skip] = got[skip]
        if got != expect:
            bad = [o for o in range(n) if got[o] != expect[o]]
            errors.append(f"{ctx}: objects {bad}: report {_hex(got)}, expected {_hex(expect)}")
        if tot != counts(expect):
            errors.append(f"{ctx}: totals {tot}, expected {counts(expect)}")
        objs_want, par_want = healed(gpu, case, before, expect)
        if skip is not None:
            objs_want[g + skip], par_want[1 + skip] = work[g + skip], par[1 + skip]
        errors += T._diffs(gpu, [(work, objs_want, g, f"{ctx}: objs"), (par, par_want, 1, f"{ctx}: parity")])
        return report, errors

    def locate_then_heal(self, gpu, le, case, work, par):
        """The call's locate then device.heal with its words, in place; the words."""
        n, g = case.n, case.guard
        lost = getattr(le.device, self.locate)(case.cls, case.params, work[g:g + n], case.size,
                                               par[1:1 + n])
        le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], lost)
        gpu.cuda.synchronize()
        return _u32(lost)

    def check_equivalence(self, gpu, le, case, dmg, room=None, arenas=None):
        """The damaged arenas twice: one through the call, one through its
        locate + device.heal.  Both arenas byte for byte and lost == report, no
        object left out.  The arenas are damaged_arenas' of the list `dmg`, or
        (dmg None) the pair `arenas`, damaged by the caller and taken over.
        Returns (the call's arenas, its report words, its totals, errors)."""
        g = case.guard
        work, par = L.damaged_arenas(gpu, case, dmg) if dmg is not None else arenas
        work2, par2 = work.clone(), par.clone()
        _, got, tot, errors = self.run_scrub(gpu, le, case, work, par, room)
        lost = self.locate_then_heal(gpu, le, case, work2, par2)
        ctx = self.ctx(case, room, f"{self.name} against {self.locate} + heal")
        if lost != got:
            errors.append(f"{ctx}: report {_hex(got)}, lost {_hex(lost)}")
        errors += T._diffs(gpu, [(work, work2, g, f"{ctx}: objs"), (par, par2, 1, f"{ctx}: parity")])
        return work, par, got, tot, errors

    def check_whole(self, gpu, le, case, blocks, room=None, composed=True):
        """scrub_helpers' whole-block damage of `blocks` through one call
        (check_scrub: the by-construction report and totals, every byte back to
        the snapshot) and, with `composed`, once more beside the call's locate
        + device.heal (check_equivalence), whose arenas are compared with the
        snapshot as well.  Returns (the first call's path, the errors)."""
        want = S.whole_words(case, blocks)
        keep = []
        work, par = S.whole_arenas(gpu, case, blocks)
        errors = ["whole blocks: " + e
                  for e in self.check_scrub(gpu, le, case, work, par, want, room=room, keep=keep)[1]]
        if composed:
            work, par, got, _, errs = self.check_equivalence(gpu, le, case, None, room,
                                                             S.whole_arenas(gpu, case, blocks))
            errors += ["whole blocks: " + e for e in errs]
            snap, par_snap = case.dev(gpu)
            ctx = self.ctx(case, room, f"whole blocks: {self.name} beside {self.locate} + heal")
            if got != want:
                errors.append(f"{ctx}: report {_hex(got)}, expected {_hex(want)}")
            errors += T._diffs(gpu, [(work, snap, case.guard, f"{ctx}: objs"),
                                     (par, par_snap, 1, f"{ctx}: parity")])
        return path(gpu, keep[0], want), errors


def healed(gpu, case, before, words):
    """The arenas a call must leave of the damaged pair `before` whose report
    is `words`: the snapshot, but a MANY object as it was damaged."""
    g = case.guard
    snap, par_snap = case.dev(gpu)
    objs_want, par_want = snap.clone(), par_snap.clone()
    for o, word in enumerate(words):
        if word == MANY:
            objs_want[g + o], par_want[1 + o] = before[0][g + o], before[1][1 + o]
    return objs_want, par_want


class Buffers:
    """The arenas, the words between their sentinels and the workspace with its
    tail of one call.  The arenas are the pair `arenas`, or the class's own,
    refilled from a damaged pair (the captured and side-stream tests, whose
    call must run on fixed addresses)."""

    def __init__(self, call, gpu, le, case, room=None, arenas=None):
        self.x, self.gpu, self.le, self.case = call, gpu, le, case
        n = case.n
        if arenas is None:
            snap, par_snap = case.dev(gpu)
            arenas = gpu.zeros_like(snap), gpu.zeros_like(par_snap)
        self.work, self.par = arenas
        self.report = gpu.full((n + 2,), L.PREFILL, dtype=gpu.int32, device="cuda")
        self.totals = gpu.full((4,), TOTALS_PREFILL, dtype=gpu.int32, device="cuda")
        self.report[0], self.report[-1] = L.SENTINELS
        self.totals[0], self.totals[3] = L.SENTINELS
        self.need = call.workspace_bytes(le, case, room)
        self.ws = gpu.full((self.need + WS_TAIL,), WS_FILL, dtype=gpu.uint8, device="cuda")

    def refill(self, src):
        self.work.copy_(src[0])
        self.par.copy_(src[1])
        self.report.fill_(L.PREFILL)
        self.report[0], self.report[-1] = L.SENTINELS
        self.totals.fill_(TOTALS_PREFILL)
        self.totals[0], self.totals[3] = L.SENTINELS

    def call(self, stream=None):
        case, n, g = self.case, self.case.n, self.case.guard
        return getattr(self.le.device, self.x.name)(
            case.cls, case.params, self.work[g:g + n], case.size, self.par[1:1 + n],
            report=self.report[1:1 + n], totals=self.totals[1:3], workspace=self.ws[:self.need],
            stream=stream)

    def tail_errors(self, ctx):
        if bool((self.ws[self.need:] == WS_FILL).all()):
            return []
        return [f"{ctx}: workspace written past its {self.need} bytes"]

    def untouched(self, src):
        """The errors of everything that no longer holds what refill put there."""
        gpu, n = self.gpu, self.case.n
        errors = T._diffs(gpu, [(self.work, src[0], self.case.guard, "objs"), (self.par, src[1], 1, "parity")])
        if _u32(self.report) != [L.SENTINELS[0]] + [L.PREFILL & 0xFFFFFFFF] * n + [L.SENTINELS[1]]:
            errors.append("report written")
        if _u32(self.totals) != [L.SENTINELS[0]] + [TOTALS_PREFILL] * 2 + [L.SENTINELS[1]]:
            errors.append("totals written")
        return errors

    def check(self, before, words, ctx):
        """The errors of a call over the damaged pair `before` whose report
        must be `words`: arenas, report and totals between their sentinels,
        the workspace's tail."""
        gpu, case = self.gpu, self.case
        o_want, p_want = healed(gpu, case, before, words)
        errors = T._diffs(gpu, [(self.work, o_want, case.guard, f"{ctx}: objs"),
                                (self.par, p_want, 1, f"{ctx}: parity")])
        got, tot = _u32(self.report), _u32(self.totals)
        if got != [L.SENTINELS[0]] + list(words) + [L.SENTINELS[1]]:
            errors.append(f"{ctx}: report {_hex(got)} (first and last: sentinels)")
        if tot != [L.SENTINELS[0]] + counts(words) + [L.SENTINELS[1]]:
            errors.append(f"{ctx}: totals {_hex(tot)} (first and last: sentinels)")
        return errors + self.tail_errors(ctx)


# gf8_heal_list: 4 SIMDs of LEOEC_GF8_HEAL_WAVES = 4 waves, wg / 64 waves a
# workgroup (scrub_impl.hpp); tiles of 4,096 bytes at 256 lanes
SCRUB = Call("scrub", "locate", False, L.FAMILIES, L.family_id, None, sizes, S.words_of, 4096,
             lambda wg: 4 * 4 * 64 // wg)
# bit_heal_list: 1 KiB of a packet per workgroup of one wave, 32 waves a compute
# unit, w KiB of its 160 KiB of LDS each (bit_heal_tile.hpp)
SCRUB_WS = Call("scrub_ws", "locate_ws", True, W.FAMILIES, W.family_id, None, sizes_and_whole,
                S.words_of, 1024, lambda w: min(160 // w, 32))
# gfw_heal_list: 4 KiB of a block per item, one wave per workgroup, 4 waves on
# each of a compute unit's 4 SIMDs (gfw_heal_tile.hpp); LAST has k + m = 31,
# the last id the report has a bit for
SCRUB_GFW = Call("scrub_gfw", "locate_gfw", True, G.FAMILIES, G.family_id, ("vandrs", 16, 15, 8, 8704),
                 sizes_and_whole, G.words_of, 4096, lambda: 16)
CALLS = (SCRUB, SCRUB_WS, SCRUB_GFW)
