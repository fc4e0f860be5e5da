"""Shared pieces of the scrub position tests (test_device_scrub_positions.py,
test_gf8_instances.py): the position batch of the edge harness
(gpu_helpers.EdgeCase), in which every block of the code is the one damaged
block of one object, the words leoec_verify_dev, leoec_locate_dev and
leoec_locate_ws_dev must answer for it by construction, the same words from
the oracle and the host models (locate_helpers, locate_ws_helpers), and one
device call each of verify, locate and heal over given arenas with every byte
and the words around the covered ones compared afterwards; and the whole-block
batch of the scrub tests (test_device_scrub.py, test_device_scrub_ws.py, the
forms modules and the instance children), in which every valid byte of the
damaged block is wrong."""
import numpy as np

import gpu_helpers as H
import heal_helpers as P
import locate_helpers as L
import locate_ws_helpers as W
import verify_helpers as V

MANY = L.MANY
HITS = 64  # damaged bytes of a damaged block (fewer where it has fewer valid bytes)

# The XOR values: a seeded permutation of 1..255.  The damaged bytes of a
# block take the first HITS values in order; the second block of the
# two-block object takes the next HITS, so that its damage is no multiple of
# the first block's.  gf8_locate splits a syndrome byte into a 3-, a 3- and a
# 2-bit group with a table each: over either run of HITS values every group
# takes every value (values_cover; the seed is chosen for that).
VALUE_SEED = 0
VALUES = (np.random.Generator(np.random.PCG64(VALUE_SEED)).permutation(255) + 1).tolist()


def values_cover(vals):
    """Every table entry of the three groups is read by some value."""
    return ({v & 7 for v in vals} == set(range(8)) and {(v >> 3) & 7 for v in vals} == set(range(8))
            and {(v >> 6) & 3 for v in vals} == set(range(4)))


def bitsliced(cls):
    return cls in ("cauchyrs", "liberation")


def block_valid(case, b):
    """Valid bytes of block b: a data block ends at `size`, a coding block is whole."""
    return case.bs if b >= case.k else H.block_valids(case.k, case.bs, case.size)[b]


def block_hits(case, b):
    """Offsets inside block b of its damaged bytes, in the order of their
    values: min(HITS, valid bytes) of them.  Even b: from the block's first
    byte; odd b: from the first byte of the last partial tile
    (verify_helpers.damage's arithmetic: 4,096-byte tiles of the block for the
    byte kernels, packet_tile of a packet for the bitmatrix classes), moved
    down where the run would leave the block (the packet).  vandrs and isars:
    consecutive bytes.  cauchyrs and liberation: byte t in packet t mod w at
    in-packet offset start + t // w, so every packet is hit.  Positions past
    the block's valid bytes are passed over and the run goes on (around the
    end of the packet) until it has its count."""
    w, bs = case.w, case.bs
    valid = block_valid(case, b)
    tile = V.packet_tile(case.cls, w)
    pw, ps, tl = (1, bs, 4096) if tile is None else (w, bs // w, tile)
    per = -(-HITS // pw)  # offsets taken of a packet (byte kernels: of the block)
    start = 0 if b % 2 == 0 else (ps - 1) // tl * tl
    start = min(start, max((ps if pw > 1 else valid) - per, 0))
    t = np.arange(pw * ps)
    pos = (t % pw) * ps + (start + t // pw) % ps
    return pos[pos < valid][:HITS].tolist()


def _entries(case, o, b, values):
    """The damage entries (locate_helpers' format) of block b of object o."""
    k, bs = case.k, case.bs
    where, base = ("objs", b * bs) if b < k else ("parity", (b - k) * bs)
    return [(where, o, base + off, x) for off, x in zip(block_hits(case, b), values)]


def position_batch(case):
    """(damage list, verify words, locate words) of a case of k + m + 2
    objects: object b < k + m has block b damaged, object k + m is clean,
    object k + m + 1 has data block 0 and coding block m - 1 damaged.  The
    words are what the damage means, not what any code answers: verify 1 << i
    for coding block i and every bit for a data block (the codes are MDS and
    every coefficient is non-zero), locate 1 << b; a data block wholly past
    `size` stays clean and its object expects 0.  The two-block object: every
    verify bit; LEOEC_LOCATE_MANY for m >= 3, None for m = 2, where the word
    is the host model's (two_block_word), and for m = 1 (no locate)."""
    k, m, n = case.k, case.m, case.n
    assert n == k + m + 2
    every = (1 << m) - 1
    dmg, verify, locate = [], [], []
    for b in range(k + m):
        hits = _entries(case, b, b, VALUES[:HITS])
        dmg += hits
        verify.append(0 if not hits else every if b < k else 1 << (b - k))
        locate.append(1 << b if hits else 0)
    verify.append(0)
    locate.append(0)
    dmg += _entries(case, n - 1, 0, VALUES[:HITS])
    dmg += _entries(case, n - 1, k + m - 1, VALUES[HITS:2 * HITS])
    verify.append(every)
    locate.append(MANY if m >= 3 else None)
    return dmg, verify, locate


def damaged_objects(case, dmg, objects=None):
    """{o: (data bytes, [m coding blocks])} as the damage leaves the touched
    objects (of `objects`); every position inside valid bytes."""
    out = {}
    for where, o, pos, x in dmg:
        if objects is not None and o not in objects:
            continue
        if o not in out:
            out[o] = L.object_blocks(case, o)
        data, stored = out[o]
        if where == "objs":
            assert 0 <= pos < case.size, (case.ident(), o, pos)
            data[pos] ^= x
        else:
            assert 0 <= pos < case.m * case.bs, (case.ident(), o, pos)
            stored[pos // case.bs][pos % case.bs] ^= x
    return out


def flags_of(oracle, case, objs):
    """leoec_verify_dev's words from the oracle for damaged objects
    ({o: (data bytes, [m coding blocks])}, damaged_objects' or whole_objects'):
    the damaged data re-encoded, bit i set where coding block i differs from
    the stored one; an object not among them is 0."""
    k, m, w = case.params
    flags = [0] * case.n
    for o, (data, stored) in objs.items():
        ref = oracle.encode(case.cls, k, m, w, data.tobytes())
        flags[o] = sum(1 << i for i in range(m) if ref[k + i] != stored[i].tobytes())
    return flags


def oracle_flags(oracle, case, dmg):
    """flags_of under a damage list."""
    return flags_of(oracle, case, damaged_objects(case, dmg))


def words_of(oracle, le, case, objs, objects=None):
    """The host model's locate words (locate_helpers.model_word, or
    locate_ws_helpers' for the bitmatrix classes) of `objects` (default: all)
    for damaged objects ({o: (data bytes, [m coding blocks])}), as {o: word};
    an object not among them is 0."""
    cfg = (case.cls,) + tuple(case.params)
    if bitsliced(case.cls):
        T = le.device.locate_bitrows(case.cls, case.params)
        word = lambda data, stored: W.model_word(oracle, cfg, data, stored, T)  # noqa: E731
    else:
        T = le.device.locate_rows(case.cls, case.params)
        word = lambda data, stored: L.model_word(oracle, cfg, case.size, data, stored, T)  # noqa: E731
    wanted = range(case.n) if objects is None else objects
    return {o: word(*objs[o]) if o in objs else 0 for o in wanted}


def model_words(oracle, le, case, dmg, objects=None):
    """words_of under a damage list."""
    return words_of(oracle, le, case, damaged_objects(case, dmg, objects), objects)


def two_block_word(oracle, le, case, dmg, locate):
    """The locate words with the two-block object's filled in from the host
    model where position_batch leaves it open (m = 2: LEOEC_LOCATE_MANY or a
    third block, the documented limit)."""
    two = case.n - 1
    if locate[two] is not None:
        return list(locate)
    word = model_words(oracle, le, case, dmg, [two])[two]
    k, m = case.k, case.m
    assert word == MANY or (word in [1 << b for b in range(k + m)] and word not in (1, 1 << (k + m - 1))), \
        (case.ident(), hex(word))
    return locate[:two] + [word]


def _hex(words):
    return [hex(x) for x in words]


# ---------------------------------------------------------------------------
# Whole-block damage.  block_hits damages at most 64 bytes of a block, so after
# a rebuild every other byte of it equals the snapshot whether the kernel wrote
# it or not.  Here every valid byte of the block is damaged: a rebuild is right
# only if it stores every tile, every lane and the ragged tail.

WHOLE_SEED = 0x5C2B


def whole_batch(case):
    """The damaged block of each object of a case of k + m + 1 objects: object
    b < k + m has block b damaged, object k + m (None) is clean."""
    assert case.n == case.k + case.m + 1
    return list(range(case.k + case.m)) + [None]


def whole_dense_batch(case):
    """Any number of objects: object o has block o mod (k + m) damaged."""
    return [o % (case.k + case.m) for o in range(case.n)]


def whole_words(case, blocks):
    """The locate words the damage means: 1 << b, or 0 for a clean object and
    for a data block that lies wholly past `size` (no byte to damage)."""
    return [1 << b if b is not None and block_valid(case, b) else 0 for b in blocks]


def whole_values(case, blocks):
    """{b: (objects whose block b is damaged, [their number, valid bytes of
    block b] XOR values in 1..255)}, seeded by the case and b; blocks with no
    valid byte are left out."""
    out = {}
    for b in sorted({b for b in blocks if b is not None}):
        valid = block_valid(case, b)
        if not valid:
            continue
        objects = [o for o, x in enumerate(blocks) if x == b]
        rng = np.random.Generator(np.random.PCG64([WHOLE_SEED, case.size, case.k, case.w, b]))
        out[b] = (objects, rng.integers(1, 256, (len(objects), valid), dtype=np.uint8))
    return out


def whole_span(case, b):
    """(arena, first byte, end) of block b's valid bytes in an object's row of
    the objs arena (a data block ends at `size`) or of the parity arena."""
    k, bs = case.k, case.bs
    if b < k:
        return "objs", b * bs, b * bs + block_valid(case, b)
    return "parity", (b - k) * bs, (b - k + 1) * bs


def whole_arenas(gpu, case, blocks):
    """Clones of the case's arenas with the damage applied, by slice."""
    g = case.guard
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    for b, (objects, values) in whole_values(case, blocks).items():
        where, lo, hi = whole_span(case, b)
        t, first = (work, g) if where == "objs" else (par, 1)
        rows = gpu.tensor([first + o for o in objects], device="cuda")
        t[rows, lo:hi] ^= gpu.from_numpy(values).cuda()
    return work, par


def whole_objects(case, blocks):
    """{o: (data bytes, [m coding blocks])} as the damage leaves the damaged
    objects (damaged_objects' format), every damaged byte inside valid bytes."""
    out = {}
    for b, (objects, values) in whole_values(case, blocks).items():
        where, lo, hi = whole_span(case, b)
        assert 0 <= lo < hi <= (case.size if where == "objs" else case.m * case.bs), (case.ident(), b)
        assert values.shape == (len(objects), hi - lo) and values.min() >= 1
        for o, x in zip(objects, values):
            assert o not in out
            data, stored = out[o] = L.object_blocks(case, o)
            if where == "objs":
                data[lo:hi] ^= x
            else:
                stored[b - case.k][:] ^= x
    return out


# ---------------------------------------------------------------------------
# One device call each, over arenas the caller damaged
# (locate_helpers.damaged_arenas).

def run_verify(gpu, le, case, work, par):
    """One device.verify, flags in a pre-filled [n + 2] tensor of which the
    call covers words 1..n.  Returns (the n covered words, error or None): the
    sentinels intact and every byte of both arenas, guard rows included, as it
    was before the call."""
    n, g = case.n, case.guard
    work_snap, par_snap = work.clone(), par.clone()
    flags = gpu.full((n + 2,), -1, dtype=gpu.int32, device="cuda")
    flags[0], flags[n + 1] = V.SENTINELS
    out = le.device.verify(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                           flags=flags[1:1 + n])
    gpu.cuda.synchronize()
    assert out.data_ptr() == flags[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in flags.cpu().tolist()]
    ctx = f"verify {case.ident()} bs {case.bs}"
    err = None
    if (got[0], got[-1]) != V.SENTINELS:
        err = f"{ctx}: sentinel words {got[0]:#x}, {got[-1]:#x}"
    err = err or (H.arena_diff(gpu, work, work_snap, g, f"{ctx}: objs") or
                  H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity"))
    return got[1:-1], err


def run_locate(gpu, le, case, work, par):
    """locate_helpers.run_locate, or locate_ws_helpers.run_locate_ws (the
    workspace device.locate_ws allocates) for the bitmatrix classes."""
    if bitsliced(case.cls):
        return W.run_locate_ws(gpu, le, case, work, par)
    return L.run_locate(gpu, le, case, work, par)


def run_heal(gpu, le, case, work, par, lost, words, skip=None):
    """One device.heal of the damaged arenas with the located words
    (lost: run_locate's [n + 2] tensor, handed over unchanged; words: its
    covered words).  Every object whose word names a block must come back to
    the snapshots byte for byte with unhealed 0; an object whose word is
    LEOEC_LOCATE_MANY stays as it was damaged and gets its word back; guard
    rows, bytes past `size` and lost itself are unchanged; unhealed lies
    between intact sentinels.  `skip`: an object left out of every comparison
    (m = 2: two damaged blocks explained by a third).  Returns the errors."""
    n, g = case.n, case.guard
    snap, par_snap = case.dev(gpu)
    want, par_want = snap.clone(), par_snap.clone()
    for o, word in enumerate(words):
        if word == MANY:
            want[g + o], par_want[1 + o] = work[g + o], par[1 + o]
    lost_before = lost.clone()
    unhealed = gpu.full((n + 2,), P.PREFILL, dtype=gpu.int32, device="cuda")
    unhealed[0], unhealed[n + 1] = P.SENTINELS
    out = le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                         lost[1:1 + n], unhealed=unhealed[1:1 + n])
    gpu.cuda.synchronize()
    assert out.data_ptr() == unhealed[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in unhealed.cpu().tolist()]
    expect = [P.SENTINELS[0]] + [word if word == MANY else 0 for word in words] + [P.SENTINELS[1]]
    if skip is not None:
        expect[1 + skip] = got[1 + skip]
        want[g + skip], par_want[1 + skip] = work[g + skip], par[1 + skip]
    ctx = f"heal {case.ident()} bs {case.bs}"
    errors = []
    if got != expect:
        errors.append(f"{ctx}: unhealed {_hex(got)}, expected {_hex(expect)} (first and last: sentinels)")
    if not gpu.equal(lost, lost_before):
        errors.append(f"{ctx}: lost was written")
    for err in (H.arena_diff(gpu, work, want, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par_want, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return errors


def check_verify(gpu, le, case, work, par, want):
    """run_verify against the by-construction words; the errors."""
    got, err = run_verify(gpu, le, case, work, par)
    errors = [err] if err else []
    if got != want:
        bad = [o for o in range(case.n) if got[o] != want[o]]
        errors.append(f"verify {case.ident()} bs {case.bs}: objects {bad} (object b: block b damaged; "
                      f"k {case.k}): flags {_hex(got)}, expected {_hex(want)}")
    return errors


def check_locate(gpu, le, case, work, par, want, skip=None):
    """run_locate against the by-construction words (`skip`: an object whose
    word is not compared).  Returns (the [n + 2] tensor, the errors)."""
    lost, got, err = run_locate(gpu, le, case, work, par)
    errors = [err] if err else []
    bad = [o for o in range(case.n) if got[o] != want[o] and o != skip]
    if bad:
        errors.append(f"locate {case.ident()} bs {case.bs}: objects {bad} (object b: block b damaged; "
                      f"k {case.k}): words {_hex(got)}, expected {_hex(want)}")
    return lost, errors
