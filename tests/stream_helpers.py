"""Shared pieces of the stream tests (test_device_streams.py): the device
calls of include/leoec.h captured into a graph and replayed, and a scrub
pipeline enqueued on a side stream with no host synchronisation inside, both on
the edge harness of gpu_helpers (guarded arenas, random non-zero bytes behind
every object, every byte of every arena compared afterwards, bit-exact with
the oracle's blocks of the EdgeCase).

Why: every other device test runs on the null stream, where a launch, a memset
or a copy that took stream 0 instead of the caller's is ordered anyway.  Under
capture such a launch is not recorded: it runs at once (or the capture fails),
so the outputs no longer hold their pre-fill when the capture ends, before any
replay; that is the deterministic check here.  A hidden allocation or a
blocking copy makes the capture itself raise.

Captured calls, per family, at the one size edge_size() (a ragged last block
and a partial last tile): a plain call first (code objects, tables), then the
capture over pre-filled outputs, then three replays over refilled buffers: the
case's batch, the batch rotated by one object, the first batch again (verify:
its two damaged batches and a clean one; heal: the masks, the masks reversed,
the masks again)."""
import numpy as np

import gpu_helpers as H
import heal_helpers as P
import locate_helpers as L
import scrub_helpers as S
import verify_helpers as V

FAMILIES = V.FAMILIES          # 15 rows: every launch shape of the device calls
HEAL_FAMILIES = P.GF8_FAMILIES + [("vandrs", 10, 4, 8, 164992)]  # the fused rows: capturable heal
WS_FILL = 0xEE                 # every workspace byte before a call
family_id = V.family_id


def edge_size(family):
    """k B - 17: a ragged last block and a partial last tile."""
    cls, k, m, w, B = family
    size = H.edge_sizes(k, w, B)[4]
    assert size == k * B - 17
    return size


def rotation(n):
    """Object o of the rotated batch holds object (o + 1) mod n."""
    return [(o + 1) % n for o in range(n)]


def rolled(arena, guard, n):
    """A copy of a [guard + n + guard, stride] arena with its object rows
    rotated by one (rotation()); guard rows as they are."""
    out = arena.clone()
    out[guard:guard + n] = arena[guard:guard + n].roll(-1, 0)
    return out


def ws_chunks(nobj, workspace_bytes, m, bs):
    """[(first object, objects)] of the chunks in which a two-pass call works
    through a batch with this workspace (ws_pass.hpp: workspace_bytes / (m bs)
    objects per chunk; the grid bound is far away at these shapes)."""
    step = workspace_bytes // (m * bs)
    assert step >= 1
    return [(o0, min(step, nobj - o0)) for o0 in range(0, nobj, step)]


def _u32(t):
    return [int(x) & 0xFFFFFFFF for x in t.cpu().tolist()]


def _hex(words):
    return [hex(x) for x in words]


def _words(gpu, n, prefill):
    """[n + 2] int32 words, `prefill` between the sentinels."""
    t = gpu.full((n + 2,), prefill - (1 << 32) if prefill >> 31 else prefill, dtype=gpu.int32,
                 device="cuda")
    t[0], t[n + 1] = V.SENTINELS
    return t


def _expect_words(n, words):
    return [V.SENTINELS[0]] + list(words) + [V.SENTINELS[1]]


class Captured:
    """One library call captured into a graph.  `call` is made once plainly
    (it loads code objects and builds tables, and `refill` has put a batch in
    place for it), then, after a device synchronisation and a refill, once
    inside torch.cuda.graph in the default capture error mode; `untouched`
    then returns the errors of every output that no longer holds its
    pre-fill.  replay(): one replay and a device synchronisation."""

    def __init__(self, gpu, call, refill, untouched):
        refill()
        call()
        gpu.cuda.synchronize()
        refill()
        gpu.cuda.synchronize()
        self.gpu = gpu
        self.graph = gpu.cuda.CUDAGraph()
        with gpu.cuda.graph(self.graph):
            call()
        gpu.cuda.synchronize()
        self.errors = [f"after the capture, before any replay: {e}" for e in untouched() if e]

    def replay(self):
        self.graph.replay()
        self.gpu.cuda.synchronize()


def _diffs(gpu, pairs):
    """The arena_diff errors of [(got, want, guard, what)]."""
    return [e for e in (H.arena_diff(gpu, *p) for p in pairs) if e]


# ---------------------------------------------------------------------------
# encode, decode, repair: the batch, the batch rotated, the batch again.

def captured_encode(gpu, le, case):
    """check_encode's comparison under capture and replay: the oracle's coding
    blocks in bytes [0, m bs) of every row of a 0x5A-filled parity arena, 0x5A
    everywhere else, the objs arena untouched.  Returns the errors."""
    m, bs, n, g = case.m, case.bs, case.n, case.guard
    snap, _ = case.dev(gpu)
    want = np.full((n, m * bs + 48), H.PARITY_FILL, dtype=np.uint8)
    want[:, :m * bs] = case.parity
    want = case.arena(gpu, want, H.PARITY_FILL)
    blank = case.arena(gpu, m * bs + 48, H.PARITY_FILL)
    batches = [(snap, want), (rolled(snap, g, n), rolled(want, 1, n)), (snap, want)]
    work, par = snap.clone(), blank.clone()
    ctx = f"captured encode {case.ident()} bs {bs}"
    src = [snap]

    def refill():
        work.copy_(src[0])
        par.copy_(blank)

    cap = Captured(gpu, lambda: le.device.encode(case.cls, case.params, work[g:g + n], case.size,
                                                 par[1:1 + n]),
                   refill, lambda: _diffs(gpu, [(par, blank, 1, f"{ctx}: parity"),
                                                (work, snap, g, f"{ctx}: objs")]))
    errors = cap.errors
    for r, (objs_in, par_want) in enumerate(batches):
        src[0] = objs_in
        refill()
        cap.replay()
        errors += _diffs(gpu, [(par, par_want, 1, f"{ctx} replay {r}: parity"),
                               (work, objs_in, g, f"{ctx} replay {r}: objs")])
    return errors


def captured_decode(gpu, le, case, erased):
    """check_decode's comparison under capture and replay, the erased coding
    blocks poisoned as well (they are no survivors: never read, never
    written).  Returns the errors."""
    k, bs, size, n, g = case.k, case.bs, case.size, case.n, case.guard
    snap, par_snap = case.dev(gpu)
    batches = [(snap, par_snap), (rolled(snap, g, n), rolled(par_snap, 1, n)), (snap, par_snap)]
    work, par = snap.clone(), par_snap.clone()
    ctx = f"captured decode {case.ident()} bs {bs} erased {list(erased)}"
    src = [batches[0]]

    def poison(objs, parity):
        for e in erased:
            if e < k:
                lo, hi = e * bs, min((e + 1) * bs, size)
                if objs is not None and lo < hi:
                    objs[g:g + n, lo:hi] = H.POISON
            else:
                parity[1:1 + n, (e - k) * bs:(e - k + 1) * bs] = H.POISON

    def refill():
        work.copy_(src[0][0])
        par.copy_(src[0][1])
        poison(work, par)

    work_poisoned, par_poisoned = snap.clone(), par_snap.clone()
    poison(work_poisoned, par_poisoned)
    assert not gpu.equal(work_poisoned, snap)  # a data block with valid bytes is erased
    cap = Captured(gpu, lambda: le.device.decode(case.cls, case.params, work[g:g + n], size,
                                                 par[1:1 + n], list(erased)),
                   refill, lambda: _diffs(gpu, [(work, work_poisoned, g, f"{ctx}: objs"),
                                                (par, par_poisoned, 1, f"{ctx}: parity")]))
    errors = cap.errors
    for r, batch in enumerate(batches):
        src[0] = batch
        refill()
        cap.replay()
        par_want = batch[1].clone()
        poison(None, par_want)
        errors += _diffs(gpu, [(work, batch[0], g, f"{ctx} replay {r}: objs"),
                               (par, par_want, 1, f"{ctx} replay {r}: parity")])
    return errors


def captured_repair(gpu, le, case, lost):
    """check_repair's comparison under capture and replay: the oracle's blocks
    in bytes [0, bs) of every row of 0x3C-filled output arenas, 0x3C everywhere
    else, the input blocks untouched.  Returns the errors."""
    k, m, bs, n = case.k, case.m, case.bs, case.n
    ctx = f"captured repair {case.ident()} bs {bs} lost {list(lost)}"
    snaps, avail = {}, []
    for b in range(k + m):
        if b in lost:
            avail.append(None)
            continue
        snaps[b] = case.arena(gpu, np.concatenate([case.blocks[b], case.slack[b]], axis=1),
                              H.GUARD_FILL)
        avail.append(snaps[b].clone())
    wants = []
    for b in lost:
        want = np.full((n, bs + 48), H.REPAIR_FILL, dtype=np.uint8)
        want[:, :bs] = case.blocks[b]
        wants.append(case.arena(gpu, want, H.REPAIR_FILL))
    blank = case.arena(gpu, bs + 48, H.REPAIR_FILL)
    outs = [blank.clone() for _ in lost]
    rot_snaps = {b: rolled(s, 1, n) for b, s in snaps.items()}
    rot_wants = [rolled(x, 1, n) for x in wants]
    batches = [(snaps, wants), (rot_snaps, rot_wants), (snaps, wants)]
    src = [snaps]

    def refill():
        for b, s in src[0].items():
            avail[b].copy_(s)
        for o in outs:
            o.copy_(blank)

    def call():
        le.device.repair(case.cls, case.params, [a if a is None else a[1:1 + n] for a in avail], bs,
                         list(lost), [o[1:1 + n] for o in outs], n)

    cap = Captured(gpu, call, refill,
                   lambda: _diffs(gpu, [(o, blank, 1, f"{ctx}: block {b}") for o, b in zip(outs, lost)] +
                                  [(avail[b], s, 1, f"{ctx}: input block {b}") for b, s in snaps.items()]))
    errors = cap.errors
    for r, (ins, want) in enumerate(batches):
        src[0] = ins
        refill()
        cap.replay()
        errors += _diffs(gpu, [(o, x, 1, f"{ctx} replay {r}: block {b}")
                               for o, x, b in zip(outs, want, lost)] +
                         [(avail[b], s, 1, f"{ctx} replay {r}: input block {b}")
                          for b, s in ins.items()])
    return errors


# ---------------------------------------------------------------------------
# verify: its two damaged batches, then a clean one.

def verify_workspace_bytes(case):
    """Bytes of the explicit workspace of a captured verify: None for the fused
    families, two objects' rows otherwise (five objects: chunks of 2, 2, 1)."""
    if V.fused(case.cls, *case.params):
        return None
    return 2 * case.m * case.bs


def verify_batches(oracle, case):
    """[(verify_helpers' damage triples, expected flag words)] of the three
    replays: both damaged batches, then an undamaged one."""
    return [(V.damage(case, False), V.expected_flags(oracle, case, False)),
            (V.damage(case, True), V.expected_flags(oracle, case, True)),
            ([], [0] * case.n)]


def captured_verify(gpu, le, oracle, case):
    """One captured device.verify, flags pre-filled with 0xFFFFFFFF between
    sentinels, the workspace (two-pass families: 2 m bs bytes, three chunks
    that reuse the same rows) with 0xEE.  After the capture the flags and the
    workspace still hold their pre-fill; every replay gives the batch's words
    and leaves both arenas as they were damaged.  Returns the errors."""
    n, g = case.n, case.guard
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    flags = _words(gpu, n, V.PREFILL)
    nbytes = verify_workspace_bytes(case)
    ws = None if nbytes is None else gpu.full((nbytes,), WS_FILL, dtype=gpu.uint8, device="cuda")
    ctx = f"captured verify {case.ident()} bs {case.bs} workspace {nbytes}"
    batches = verify_batches(oracle, case)
    src = [batches[0][0]]

    def refill():
        work.copy_(snap)
        par.copy_(par_snap)
        for where, o, pos in src[0]:
            row = work[g + o] if where == "objs" else par[1 + o]
            row[pos] ^= V.BIT
        flags[1:1 + n] = -1
        if ws is not None:
            ws.fill_(WS_FILL)

    def untouched():
        got = _u32(flags)
        errs = []
        if got != _expect_words(n, [V.PREFILL] * n):
            errs.append(f"{ctx}: flags {_hex(got)}")
        if ws is not None and not bool((ws == WS_FILL).all()):
            errs.append(f"{ctx}: {int((ws != WS_FILL).sum())} workspace bytes written")
        return errs

    cap = Captured(gpu, lambda: le.device.verify(case.cls, case.params, work[g:g + n], case.size,
                                                 par[1:1 + n], flags=flags[1:1 + n], workspace=ws),
                   refill, untouched)
    errors = cap.errors
    for r, (dmg, want) in enumerate(batches):
        src[0] = dmg
        refill()
        work_before, par_before = work.clone(), par.clone()
        cap.replay()
        got = _u32(flags)
        if got != _expect_words(n, want):
            errors.append(f"{ctx} replay {r}: flags {_hex(got)}, expected "
                          f"{_hex(_expect_words(n, want))} (first and last: sentinels)")
        errors += _diffs(gpu, [(work, work_before, g, f"{ctx} replay {r}: objs"),
                               (par, par_before, 1, f"{ctx} replay {r}: parity")])
    return errors


# ---------------------------------------------------------------------------
# heal (fused rows): the masks, the masks reversed, the masks again.

def heal_batch(gpu, case, masks):
    """heal_helpers.run_heal's arenas for `masks`: (objs and parity with the
    lost blocks poisoned, data blocks only up to `size`; what a heal must
    leave of them: the snapshots for a recoverable object, the poison for an
    unrecoverable one; the unhealed words)."""
    k, m, bs, size, n, g = case.k, case.m, case.bs, case.size, case.n, case.guard
    assert len(masks) == n
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    want, par_want = snap.clone(), par_snap.clone()
    for o, mask in enumerate(masks):
        healed = P.recoverable(mask, k, m)
        for b in P.ids_of(mask):
            if b < k:
                lo, hi = b * bs, min((b + 1) * bs, size)
                if lo < hi:
                    work[g + o, lo:hi] = H.POISON
                    if not healed:
                        want[g + o, lo:hi] = H.POISON
            elif b < k + m:
                lo = (b - k) * bs
                par[1 + o, lo:lo + bs] = H.POISON
                if not healed:
                    par_want[1 + o, lo:lo + bs] = H.POISON
    words = [0 if P.recoverable(mk, k, m) else mk for mk in masks]
    return work, par, want, par_want, words


def captured_heal(gpu, le, case, masks):
    """One captured device.heal of a fused family; `lost` is rewritten between
    the replays (the masks, the masks reversed, the masks again), unhealed
    pre-filled between sentinels.  After the capture both arenas still hold
    their poison and unhealed its pre-fill.  Returns the errors."""
    assert P.fused(case.cls, *case.params)
    n, g = case.n, case.guard
    batches = [(mk, heal_batch(gpu, case, mk)) for mk in (masks, masks[::-1], masks)]
    work, par = batches[0][1][0].clone(), batches[0][1][1].clone()
    lost = gpu.zeros((n,), dtype=gpu.int32, device="cuda")
    unhealed = _words(gpu, n, P.PREFILL)
    ctx = f"captured heal {case.ident()} bs {case.bs}"
    src = [batches[0]]

    def refill():
        mk, (w0, p0, _, _, _) = src[0]
        work.copy_(w0)
        par.copy_(p0)
        lost.copy_(gpu.from_numpy(np.array(mk, dtype=np.uint32).view(np.int32).copy()))
        unhealed[1:1 + n] = P.PREFILL

    def untouched():
        got = _u32(unhealed)
        errs = _diffs(gpu, [(work, batches[0][1][0], g, f"{ctx}: objs"),
                            (par, batches[0][1][1], 1, f"{ctx}: parity")])
        if got != _expect_words(n, [P.PREFILL] * n):
            errs.append(f"{ctx}: unhealed {_hex(got)}")
        return errs

    cap = Captured(gpu, lambda: le.device.heal(case.cls, case.params, work[g:g + n], case.size,
                                               par[1:1 + n], lost, unhealed=unhealed[1:1 + n]),
                   refill, untouched)
    errors = cap.errors
    for r, batch in enumerate(batches):
        mk, (_, _, want, par_want, words) = batch
        src[0] = batch
        refill()
        cap.replay()
        got = _u32(unhealed)
        if got != _expect_words(n, words):
            errors.append(f"{ctx} replay {r}: unhealed {_hex(got)}, expected "
                          f"{_hex(_expect_words(n, words))} (first and last: sentinels)")
        if _u32(lost) != list(mk):
            errors.append(f"{ctx} replay {r}: lost was written")
        errors += _diffs(gpu, [(work, want, g, f"{ctx} replay {r}: objs"),
                               (par, par_want, 1, f"{ctx} replay {r}: parity")])
    return errors


# ---------------------------------------------------------------------------
# The scrub pipeline on a side stream.

WINDOW_BYTES = 512 << 20  # the fill in front of the pipeline: its copies are still queued behind it


def run_blocks(k, m):
    """heal_helpers.run_masks as damage to be found: the one damaged block of
    each of RUN_N objects (None: clean), with run_masks' runs (3, 2, 2, 2, 1,
    2 objects): the last data block, clean, data block 0, coding block 0, the
    last coding block, the last data block again."""
    return [k - 1] * 3 + [None] * 2 + [0] * 2 + [k] * 2 + [k + m - 1] + [k - 1] * 2


def pipeline_damage(case, blocks):
    """(damage list, verify words, locate words): scrub_helpers.position_batch's
    entries and by-construction words for one damaged block per object."""
    k, m = case.k, case.m
    assert len(blocks) == case.n
    dmg, verify, locate = [], [], []
    for o, b in enumerate(blocks):
        hits = [] if b is None else S._entries(case, o, b, S.VALUES[:S.HITS])
        dmg += hits
        verify.append(0 if not hits else (1 << m) - 1 if b < k else 1 << (b - k))
        locate.append(1 << b if hits else 0)
    return dmg, verify, locate


def run_pipeline(gpu, le, case, blocks):
    """verify, locate_gfw, heal and verify again on a non-blocking side
    stream, behind a large fill and the copies that bring the damaged batch
    into the work buffers, with nothing but the stream's own synchronisation
    at the end (heal's generic path waits for its masks inside the call).  A
    plain pass on the null stream comes first: code objects and tables.
    Returns the errors: the first flags and the located words are the
    damage's, heal leaves the snapshots byte for byte with unhealed 0, the
    second flags are 0, every word vector between intact sentinels."""
    cls, params, size, n, g, bs = case.cls, case.params, case.size, case.n, case.guard, case.bs
    dev = le.device
    snap, par_snap = case.dev(gpu)
    dmg, verify_want, locate_want = pipeline_damage(case, blocks)
    dwork, dpar = L.damaged_arenas(gpu, case, dmg)
    need_v = dev.verify_workspace(cls, params, size, n)
    need_l = dev.locate_gfw_workspace(cls, params, size, n)
    ws_v = gpu.full((need_v,), WS_FILL, dtype=gpu.uint8, device="cuda") if need_v else None
    ws_l = gpu.full((need_l,), WS_FILL, dtype=gpu.uint8, device="cuda") if need_l else None

    def calls(work, par, flags1, lost, unhealed, flags2):
        objs, parity = work[g:g + n], par[1:1 + n]
        dev.verify(cls, params, objs, size, parity, flags=flags1[1:1 + n], workspace=ws_v)
        dev.locate_gfw(cls, params, objs, size, parity, lost=lost[1:1 + n], workspace=ws_l)
        dev.heal(cls, params, objs, size, parity, lost[1:1 + n], unhealed=unhealed[1:1 + n])
        dev.verify(cls, params, objs, size, parity, flags=flags2[1:1 + n], workspace=ws_v)

    def words():
        return (_words(gpu, n, V.PREFILL), _words(gpu, n, L.PREFILL), _words(gpu, n, P.PREFILL),
                _words(gpu, n, V.PREFILL))

    calls(dwork.clone(), dpar.clone(), *words())  # the plain pass
    work, par = gpu.zeros_like(snap), gpu.zeros_like(par_snap)
    flags1, lost, unhealed, flags2 = words()
    scratch = gpu.empty((WINDOW_BYTES,), dtype=gpu.uint8, device="cuda")
    side = gpu.cuda.Stream()
    assert side.cuda_stream != 0 and side != gpu.cuda.default_stream()
    gpu.cuda.synchronize()  # the buffers above were filled on the null stream
    with gpu.cuda.stream(side):
        scratch.fill_(0x11)
        work.copy_(dwork)
        par.copy_(dpar)
        calls(work, par, flags1, lost, unhealed, flags2)
    side.synchronize()
    ctx = f"pipeline {case.ident()} bs {bs}"
    errors = []
    for name, t, want in (("first flags", flags1, verify_want), ("located words", lost, locate_want),
                          ("unhealed", unhealed, [0] * n), ("second flags", flags2, [0] * n)):
        got = _u32(t)
        if got != _expect_words(n, want):
            errors.append(f"{ctx}: {name} {_hex(got)}, expected {_hex(_expect_words(n, want))} "
                          "(first and last: sentinels)")
    return errors + _diffs(gpu, [(work, snap, g, f"{ctx}: objs"), (par, par_snap, 1, f"{ctx}: parity")])
