"""leoec_locate_gfw_dev on the device: the one damaged block of every object of
damaged batches of the GF(2^w) word classes (vandrs w = 16 / 32; vandrs and
isars w = 8 with k > 16 or m > 4), word for word, on the edge harness of
gpu_helpers (guarded arenas, random non-zero bytes behind every object, every
byte of every arena compared afterwards: the call writes nothing but its words
and its workspace).

Edge harness: locate_gfw_helpers.FAMILIES at every size of edge_sizes (B =
8,704: two whole 4 KiB tiles of gfw_locate and a ragged one of 512 bytes; the
small sizes a single 16-byte chunk per block).  Per (family, size) the three
calls of locate_helpers.expected_calls over EDGE_N = 5 objects, held against
the host model of locate_gfw_helpers as well; the third call's words then go
into leoec_heal_dev unchanged.  Then: the high bits of a word (the reduction
taps), every block position of five codes (the largest table, and k + m = 32),
two damaged blocks in one word column, whole damaged blocks, chunked
workspaces, forwarding, a captured graph and a pending HIP error.

Last, three objects whose rows lie 2^32 + 48 bytes apart, on the layout, the
arena and the comparison of tests/wide_helpers.py (unedited; its own
plan_locate names the two older calls and their host models, so the plan is
built here from its pieces)."""
import itertools

import numpy as np
import pytest

import gpu_helpers as H
import locate_gfw_helpers as G
import locate_helpers as L
import locate_ws_helpers as W
import scrub_helpers as S
import test_pending_hip_error as PE
import wide_helpers as Wd


@pytest.fixture(scope="module", params=G.FAMILIES, ids=G.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def _cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in H.edge_sizes(k, w, B):
        yield H.edge_case(le, oracle, family[:4], size)


def _hex(words):
    return [hex(x) for x in words]


@pytest.mark.gpu
def test_device_locate_gfw_words(gpu, le, oracle, family):
    """The exact words of the three damaged batches of every size, which are
    the host model's too; sentinels intact, every covered word overwritten,
    objs and parity arenas byte-identical to the damaged snapshots."""
    errors = []
    for case in _cases(le, oracle, family):
        for call, (dmg, want) in enumerate(L.expected_calls(case)):
            assert G.model_words(oracle, le, case, dmg) == want, (case.ident(), call)
            work, par = L.damaged_arenas(gpu, case, dmg)
            _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
            if err:
                errors.append(err)
            if got != want:
                errors.append(f"locate_gfw {case.ident()} bs {case.bs} call {1 + call}: words "
                              f"{_hex(got)}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_gfw_partial_batch(gpu, le, oracle, family):
    """nobj = n - 2 with object n - 1 damaged as well: the words of objects
    n - 2 and n - 1 keep their pre-fill."""
    errors = []
    for case in _cases(le, oracle, family):
        n = case.n
        dmg, want = L.expected_calls(case)[0]
        work, par = L.damaged_arenas(gpu, case, dmg + [("parity", n - 1, 0, L.BIT)])
        _, got, err = G.run_locate_gfw(gpu, le, case, work, par, nobj=n - 2)
        want = want[:n - 2] + [L.PREFILL] * 2
        if err:
            errors.append(err)
        if got != want:
            errors.append(f"{case.ident()}: words {_hex(got)}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_gfw_chunked_workspace(gpu, le, oracle, family):
    """The same words with a workspace of the query's size (one pass), of
    exactly m bs bytes (five chunks) and of 3 m bs (chunks of three and two
    objects)."""
    errors = []
    for case in _cases(le, oracle, family):
        n, m, bs = case.n, case.m, case.bs
        assert le.device.locate_gfw_workspace(case.cls, case.params, case.size, n) == n * m * bs
        dmg, want = L.expected_calls(case)[2]
        work, par = L.damaged_arenas(gpu, case, dmg)
        got = []
        for nbytes in (n * m * bs, m * bs, 3 * m * bs):
            ws = gpu.full((nbytes,), 0xEE, dtype=gpu.uint8, device="cuda")
            _, words, err = G.run_locate_gfw(gpu, le, case, work, par, workspace=ws)
            if err:
                errors.append(err)
            got.append(words)
        if any(words != want for words in got):
            errors.append(f"{case.ident()}: one pass {_hex(got[0])}, five chunks {_hex(got[1])}, "
                          f"two chunks {_hex(got[2])}, expected {_hex(want)}")
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_locate_gfw_heal_round_trip(gpu, le, oracle, family):
    """The third batch located, its words handed to device.heal as they are:
    objects 0 and 3 come back to the originals byte for byte (unhealed 0),
    objects 1 and 2 are untouched (unhealed == LEOEC_LOCATE_MANY), and a
    second locate_gfw finds objects 0, 3 and 4 consistent."""
    errors = []
    for case in _cases(le, oracle, family):
        n, g = case.n, case.guard
        dmg, want = L.expected_calls(case)[2]
        assert want == [1 << 0, L.MANY, L.MANY, 1 << L.last_block(case), 0]
        work, par = L.damaged_arenas(gpu, case, dmg)
        lost, got, err = G.run_locate_gfw(gpu, le, case, work, par)
        ctx = f"{case.ident()} bs {case.bs}"
        if err or got != want:
            errors.append(f"{ctx}: locate_gfw {_hex(got)}, expected {_hex(want)} {err or ''}")
            continue
        snap, par_snap = case.dev(gpu)
        healed_objs, healed_par = work.clone(), par.clone()  # what heal must leave
        for o in (0, 3):
            healed_objs[g + o] = snap[g + o]
        unhealed = le.device.heal(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                                  lost[1:1 + n])
        gpu.cuda.synchronize()
        left = [int(x) & 0xFFFFFFFF for x in unhealed.cpu().tolist()]
        if left != [0, L.MANY, L.MANY, 0, 0]:
            errors.append(f"{ctx}: unhealed {_hex(left)}")
        err = (H.arena_diff(gpu, work, healed_objs, g, f"heal {ctx}: objs") or
               H.arena_diff(gpu, par, healed_par, 1, f"heal {ctx}: parity"))
        if err:
            errors.append(err)
        _, again, err = G.run_locate_gfw(gpu, le, case, work, par)
        if err or again != [0, L.MANY, L.MANY, 0, 0]:
            errors.append(f"{ctx}: second locate_gfw {_hex(again)} {err or ''}")
    assert not errors, "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# The high bits of a word: the reduction taps of the multiply.

@pytest.mark.gpu
@pytest.mark.parametrize("family", G.FAMILIES[:3], ids=G.family_id)
def test_high_and_low_bits_of_a_word(gpu, le, oracle, family):
    """Object 0: the top bit of the highest byte of a word of a data block
    (w = 32: byte 3; w = 16: byte 1), which every doubling step reduces;
    object 1: the low bit of a word's lowest byte; object 2: both in one word
    of a coding block."""
    cls, k, m, w, B = family
    case = H.edge_case(le, oracle, family[:4], H.edge_sizes(k, w, B)[1])
    bs, wb = case.bs, w // 8
    word = 4096 + 8 * wb  # a word of the second tile
    ja, jb = k - 2, 1
    dmg = [("objs", 0, ja * bs + word + wb - 1, 0x80), ("objs", 1, jb * bs + word, 0x01),
           ("parity", 2, bs + word + wb - 1, 0x80), ("parity", 2, bs + word, 0x01)]
    want = [1 << ja, 1 << jb, 1 << (k + 1), 0, 0]
    assert G.model_words(oracle, le, case, dmg) == want
    work, par = L.damaged_arenas(gpu, case, dmg)
    _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
    assert not err, err
    assert got == want, (_hex(got), _hex(want))


# ---------------------------------------------------------------------------
# Every block position.

POSITION_CODES = [("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32), ("vandrs", 20, 4, 8),
                  ("vandrs", 16, 15, 8), ("vandrs", 28, 4, 8)]
POSITION_B = 4608  # a whole 4 KiB tile and a ragged one of 512 bytes; a multiple of 16 w


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", POSITION_CODES, ids=str)
def test_every_block_position(gpu, le, oracle, cfg):
    """scrub_helpers.position_batch: object b has block b damaged in 64 bytes
    with 64 different values (even b: from the block's first byte; odd b: in
    its ragged tile), so every ratio T[i][j] decides one object's word;
    object k + m is clean, object k + m + 1 has two damaged blocks (MANY: every
    code here has m >= 3).  (16,15,8) has the largest table, 224 ratios; at
    (28,4,8) block 31's word is LEOEC_LOCATE_MANY's own 0x80000000."""
    cls, k, m, w = cfg
    assert G.word_class(*cfg) and m >= 3
    case = H.edge_case(le, oracle, cfg, k * POSITION_B - 1, n=k + m + 2)
    assert case.bs == POSITION_B
    dmg, _, want = S.position_batch(case)
    assert want == [1 << b for b in range(k + m)] + [0, L.MANY]
    if k + m == 32:
        assert want[31] == L.MANY == 0x80000000
    assert G.model_words(oracle, le, case, dmg) == want
    work, par = L.damaged_arenas(gpu, case, dmg)
    _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
    assert not err, err
    bad = [o for o in range(case.n) if got[o] != want[o]]
    assert not bad, (bad, _hex(got))


# ---------------------------------------------------------------------------
# Two damaged blocks in one word column.

def _pairs_case(le, oracle, cfg):
    """One object per pair of blocks, at the smallest block (bs = 16 w)."""
    cls, k, m, w = cfg
    pairs = list(itertools.combinations(range(k + m), 2))
    case = H.edge_case(le, oracle, cfg, 16 * w * k, n=len(pairs))
    assert case.bs == 16 * w
    rng = np.random.Generator(np.random.PCG64(k * 100 + w))
    dmg = []
    for o, (a, b) in enumerate(pairs):
        col = int(rng.integers(0, case.bs // (w // 8)))  # the word column (128 of them)
        for blk in (a, b):
            byte = col * (w // 8) + int(rng.integers(0, w // 8))
            where, base = ("objs", blk * case.bs) if blk < k else ("parity", (blk - k) * case.bs)
            dmg.append((where, o, base + byte, int(rng.integers(1, 256))))
    return case, pairs, dmg


@pytest.mark.gpu
def test_two_blocks_in_one_word_column(gpu, le, oracle):
    """m >= 3: LEOEC_LOCATE_MANY for every pair of blocks of vandrs(6,3,32).
    m = 2, vandrs(4,2,16): the host model's words, whatever they are (the
    documented limit: MANY or a third block)."""
    for cfg in (("vandrs", 6, 3, 32), ("vandrs", 4, 2, 16)):
        cls, k, m, w = cfg
        case, pairs, dmg = _pairs_case(le, oracle, cfg)
        model = G.model_words(oracle, le, case, dmg)
        if m >= 3:
            want = [L.MANY] * len(pairs)
            assert model == want
        else:
            want = model
            for (a, b), word in zip(pairs, want):
                assert word == L.MANY or word in [1 << c for c in range(k + m) if c not in (a, b)]
        work, par = L.damaged_arenas(gpu, case, dmg)
        _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
        assert not err, err
        assert got == want, (cfg, _hex(got), _hex(want))


# ---------------------------------------------------------------------------
# Rebuild-scale damage: every valid byte of a block wrong.

@pytest.mark.gpu
def test_whole_blocks_damaged(gpu, le, oracle, family):
    """scrub_helpers' whole-block damage: the ragged last data block, the last
    coding block (the twin of multi_damage's object 3), data block 0 and
    coding block 0, every valid byte XORed with a random non-zero byte."""
    cls, k, m, w, B = family
    case = H.edge_case(le, oracle, family[:4], H.edge_sizes(k, w, B)[1])
    blocks = [k - 1, k + m - 1, 0, k, None]
    want = S.whole_words(case, blocks)
    assert want == [1 << (k - 1), 1 << (k + m - 1), 1, 1 << k, 0]
    assert G.words_of(oracle, le, case, S.whole_objects(case, blocks)) == want
    work, par = S.whole_arenas(gpu, case, blocks)
    _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
    assert not err, err
    assert got == want, (_hex(got), _hex(want))


# ---------------------------------------------------------------------------
# Forwarding.

@pytest.mark.gpu
@pytest.mark.parametrize("family", [H.EDGE_FAMILIES[0], W.FAMILIES[1]], ids=G.family_id)
def test_device_locate_gfw_forwards(gpu, le, oracle, family):
    """vandrs(10,4,8) (fused, no workspace) and cauchyrs(6,3,4) (bitmatrix):
    the query and the words are device.locate_ws'."""
    cls, k, m, w, B = family
    assert W.served(cls, k, m, w) and not G.word_class(cls, k, m, w)
    for size in H.edge_sizes(k, w, B)[:2]:
        case = H.edge_case(le, oracle, family[:4], size)
        assert le.device.locate_gfw_workspace(cls, case.params, size, case.n) == \
            le.device.locate_ws_workspace(cls, case.params, size, case.n)
        for dmg, want in L.expected_calls(case):
            work, par = L.damaged_arenas(gpu, case, dmg)
            _, ref, err = W.run_locate_ws(gpu, le, case, work, par)
            assert not err, err
            _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
            assert not err, err
            assert got == ref == want, (case.ident(), _hex(got), _hex(ref), _hex(want))


# ---------------------------------------------------------------------------
# A captured graph.

@pytest.mark.gpu
@pytest.mark.parametrize("family", G.FAMILIES[:3], ids=G.family_id)
def test_device_locate_gfw_graph(gpu, le, oracle, family):
    """The call allocates nothing and never synchronises: after one plain call
    (which builds the code's table and loads the code object) it is captured
    into a graph over a batch of 5 and replayed twice, over the batch it was
    captured on and over one damaged afterwards in the same buffers."""
    cls, k, m, w, B = family
    case = H.edge_case(le, oracle, family[:4], H.edge_sizes(k, w, B)[1])
    n, g = case.n, case.guard
    calls = L.expected_calls(case)
    work, par = L.damaged_arenas(gpu, case, calls[0][0])
    _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
    assert not err and got == calls[0][1], (err, _hex(got))
    lost = gpu.full((n,), L.PREFILL, dtype=gpu.int32, device="cuda")
    ws = gpu.full((le.device.locate_gfw_workspace(cls, case.params, case.size, n),), 0xEE,
                  dtype=gpu.uint8, device="cuda")
    gpu.cuda.synchronize()
    graph = gpu.cuda.CUDAGraph()
    with gpu.cuda.graph(graph):
        le.device.locate_gfw(cls, case.params, work[g:g + n], case.size, par[1:1 + n], lost=lost,
                             workspace=ws)
    graph.replay()
    gpu.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()] == calls[0][1]
    # the same buffers holding the third batch
    work3, par3 = L.damaged_arenas(gpu, case, calls[2][0])
    work.copy_(work3)
    par.copy_(par3)
    lost.fill_(L.PREFILL)
    ws.fill_(0xEE)
    graph.replay()
    gpu.cuda.synchronize()
    assert [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()] == calls[2][1]


# ---------------------------------------------------------------------------
# A HIP error pending on the calling thread (test_pending_hip_error.py's way).

@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [("vandrs", 6, 3, 32), ("vandrs", 20, 4, 8)], ids=str)
def test_device_locate_gfw_with_pending_error(gpu, le, oracle, cfg):
    """With hipErrorInvalidDevice planted on the thread the call returns
    LEOEC_OK with the right words and leaves the error in place."""
    hip = PE.Runtime(le)
    case = PE._case(le, oracle, *cfg)
    dmg = L.with_bit(PE.V.damage(case, False))
    want = G.model_words(oracle, le, case, dmg)
    assert want == [1 << case.k, 1 << (case.k + case.m - 1), 1 << L.last_block(case)]
    work, par = L.damaged_arenas(gpu, case, dmg)
    # a first call: the table and the code object
    _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
    assert not err and got == want, (err, _hex(got))
    try:
        with PE.planted(gpu, le, hip, "leoec_locate_gfw_dev") as calls:
            _, got, err = G.run_locate_gfw(gpu, le, case, work, par)
    finally:
        hip.get()
    PE._check_calls(calls, "leoec_locate_gfw_dev")
    assert not err, err
    assert got == want, (_hex(got), _hex(want))
    assert hip.peek() == PE.HIP_SUCCESS


# ---------------------------------------------------------------------------
# Rows more than 4 GiB apart (wide_helpers: three objects, STRIDE = 2^32 + 48).

WIDE_FAMILY = ("vandrs", 6, 3, 32, 8704)


def wide_plan(le, oracle, variant):
    """wide_helpers.plan_locate for device.locate_gfw: object 0 clean, the
    ragged last data block of object 1 and the first coding block of object 2
    wholly damaged; "query": the query's workspace (one pass), "one": one
    object's (the chunk loop's host-side o0 * stride)."""
    assert WIDE_FAMILY in Wd.FAMILIES and G.word_class(*WIDE_FAMILY[:4])
    case, lay = Wd.wide_case(le, oracle, WIDE_FAMILY), Wd.layout(le, WIDE_FAMILY)
    m, bs, n = case.m, case.bs, Wd.NOBJ
    blocks = Wd.locate_blocks(case)
    p = Wd.Plan(case, lay, "locate_gfw", variant)
    p.pre = Wd._base(lay, case)
    Wd._damage(lay, case, p.pre, blocks)
    p.want = Wd._copy(p.pre)
    want = S.whole_words(case, blocks)
    assert want == [0, 1 << (case.k - 1), 1 << case.k]
    assert G.words_of(oracle, le, case, S.whole_objects(case, blocks)) == want
    p.words_pre = {"lost": Wd._sentinels([L.PREFILL] * n, L.SENTINELS)}
    p.words_want = {"lost": Wd._sentinels(want, L.SENTINELS), "workspace tail": Wd.WS_TAIL_WANT}
    need = le.device.locate_gfw_workspace(case.cls, case.params, case.size, n)
    assert need == n * m * bs
    need = m * bs if variant == "one" else need
    p.model = lambda objs: {"lost": Wd._sentinels(G.words_of(oracle, le, case, objs), L.SENTINELS)}

    def run(gpu, le, arena, words):
        objs, par = Wd._views(arena, lay, case)
        lost = Wd._i32(gpu, words["lost"])
        ws = Wd._workspace(gpu, need)
        le.device.locate_gfw(case.cls, case.params, objs, case.size, par, lost=lost[1:1 + n],
                             workspace=ws[:need])
        gpu.cuda.synchronize()
        return {"lost": Wd.D._u32(lost), "workspace tail": Wd._tail(ws, need)}
    p.run = run
    return p


def test_wide_compare_can_fail(le, oracle):
    """No GPU: the comparison finds nothing in what the expectation itself
    holds, and names row 1 or row 2 in what a kernel leaves that kept a row
    offset or a stride in 32 bits (wide_helpers.simulate: the call writes no
    region, so its words tell)."""
    p = wide_plan(le, oracle, "query")
    assert Wd.compare(p.lay, p.want, p.want) == [] and Wd.compare_words(p.words_want, p.words_want) == []
    for name, trunc in Wd.truncations():
        got, words = Wd.simulate(p, trunc)
        assert Wd.compare(p.lay, got, p.want) == []
        errors = Wd.compare_words(words, p.words_want)
        assert any("row 1" in e or "row 2" in e for e in errors), (name, errors, words)


@pytest.mark.gpu
def test_device_locate_gfw_wide_strides(gpu, le, oracle):
    """vandrs(6,3,32) on three objects whose objs and parity rows lie
    2^32 + 48 bytes apart in one device allocation: the words, every byte of
    both regions of every row widened by 4 KiB, and the bytes behind the
    workspace, with the query's workspace and with one object's."""
    lay = Wd.layout(le, WIDE_FAMILY)
    arena = Wd.Arena(gpu, lay.used)
    try:
        errors = []
        for variant in ("query", "one"):
            errors += Wd.execute(gpu, le, arena, wide_plan(le, oracle, variant))
        assert not errors, "\n".join(errors[:12])
    finally:
        arena.release()
