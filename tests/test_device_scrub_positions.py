"""The device scrub path with every block position damaged in turn: verify,
locate, heal and a second locate over the position batch of scrub_helpers, on
the edge harness of gpu_helpers (guarded arenas, random non-zero bytes behind
every object, every byte of both arenas and the words around the covered ones
compared after every call).

The other device tests damage coding blocks 0 and m-1 and data blocks 0, 1
and the last one, nearly always with the one bit 0x10.  Here object b of a
batch of k + m + 2 has block b damaged, for every b: up to 64 bytes with 64
different XOR values that between them read every entry of gf8_locate's three
perm tables, at the block's first byte (even b) or in its last partial tile
(odd b), across every packet for the bitmatrix classes.  So every ratio table
T[i][j] of gf8_locate and of bit_locate decides one object's word, every flag
bit of verify is set alone once, and heal rebuilds every block once from the
located word.  Object k + m is clean; object k + m + 1 has two damaged blocks.

Families: locate_helpers.FAMILIES through device.locate, locate_ws_helpers.
FAMILIES through device.locate_ws, and the remaining rows of
verify_helpers.FAMILIES (the two-pass GF(2^w) shapes) for verify alone.  Two
sizes of edge_sizes each: k B - 1 (whole and partial tiles, the last block one
byte short) and 16 w (k - 2) + 5 (the last block empty, the one before it five
bytes).  Expected words are scrub_helpers.position_batch's, by construction;
the CPU test below holds them against the oracle and the host models."""
import pytest

import gpu_helpers as H
import locate_helpers as L
import locate_ws_helpers as W
import scrub_helpers as S
import verify_helpers as V

FAMILIES = V.FAMILIES + [f for f in L.FAMILIES if f not in V.FAMILIES]


def locatable(family):
    return family in L.FAMILIES or family in W.FAMILIES


def sizes(family):
    cls, k, m, w, B = family
    out = [k * B - 1, 16 * w * (k - 2) + 5]
    assert all(s in H.edge_sizes(k, w, B) for s in out)
    return out


@pytest.fixture(scope="module", params=FAMILIES, ids=V.family_id)
def family(request):
    return request.param


def _cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in sizes(family):
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 2)


def test_family_table(le):
    """Every family of the verify, locate and locate_ws tests once; the
    locatable ones are exactly those the two calls serve; the two sizes are
    what they claim."""
    assert len(FAMILIES) == len(set(FAMILIES)) == 16
    assert set(FAMILIES) == set(V.FAMILIES) | set(L.FAMILIES) | set(W.FAMILIES)
    for f in FAMILIES:
        cls, k, m, w, B = f
        assert locatable(f) == W.served(cls, k, m, w), f
        (big, bs0), (small, bs1) = [(s, le.layout(cls, (k, m, w), s)[0]) for s in sizes(f)]
        assert bs0 == B and H.block_valids(k, bs0, big)[-2:] == [B, B - 1]
        assert bs1 == 16 * w and H.block_valids(k, bs1, small)[-3:] == [bs1, 5, 0]


def test_values_read_every_table_entry():
    """A condition on the inputs: over the 64 values of a damaged block (and
    over the next 64, the second block of the two-block object) the groups
    v & 7, (v >> 3) & 7 and (v >> 6) & 3 take every value."""
    assert sorted(S.VALUES) == list(range(1, 256))
    assert S.values_cover(S.VALUES[:S.HITS]) and S.values_cover(S.VALUES[S.HITS:2 * S.HITS])
    assert not set(S.VALUES[:S.HITS]) & set(S.VALUES[S.HITS:2 * S.HITS])


def test_position_batch_against_oracle_and_model(le, oracle, family):
    """No GPU: for every case of the GPU test the damage lies inside valid
    bytes (damaged_objects asserts that), every damaged block has
    min(64, valid) damaged bytes at distinct places, the oracle's re-encoding
    gives the by-construction flags, and the host model the by-construction
    words (for the two-block object of an m = 2 code: MANY or a third block)."""
    cls, k, m, w, B = family
    for case in _cases(le, oracle, family):
        dmg, verify, locate = S.position_batch(case)
        assert len({(wh, o, p) for wh, o, p, _ in dmg}) == len(dmg)
        for b in range(k + m):
            hits = S.block_hits(case, b)
            assert len(hits) == min(S.HITS, S.block_valid(case, b)), (case.ident(), b)
            assert (verify[b] != 0) == bool(hits)
            if bool(hits) and S.bitsliced(cls) and S.block_valid(case, b) == case.bs:
                assert {p // (case.bs // w) for p in hits} == set(range(w))  # every packet
        assert verify[k + m - 1] == 1 << (m - 1) and verify[-2:] == [0, (1 << m) - 1]
        assert S.oracle_flags(oracle, case, dmg) == verify, case.ident()
        if not locatable(family):
            continue
        model = S.model_words(oracle, le, case, dmg)
        want = S.two_block_word(oracle, le, case, dmg, locate)
        assert [model[o] for o in range(case.n)] == want, case.ident()
        assert want[-1] == S.MANY or m == 2


@pytest.mark.gpu
def test_device_scrub_positions(gpu, le, oracle, family):
    """verify, locate, heal with the located words as they are, locate again:
    the by-construction words; every named object back to the snapshots byte
    for byte with unhealed 0, the two-block object untouched with its word
    returned; the second locate all zero but for that object."""
    cls, k, m, w, B = family
    errors = []
    for case in _cases(le, oracle, family):
        dmg, verify, locate = S.position_batch(case)
        work, par = L.damaged_arenas(gpu, case, dmg)
        errors += S.check_verify(gpu, le, case, work, par, verify)
        if not locatable(family):
            continue
        want = S.two_block_word(oracle, le, case, dmg, locate)
        lost, errs = S.check_locate(gpu, le, case, work, par, want)
        errors += errs
        if errs:
            continue  # heal takes the words as they are: not with wrong ones
        skip = None if want[-1] == S.MANY else case.n - 1
        errors += S.run_heal(gpu, le, case, work, par, lost, want, skip)
        again = [0] * (case.n - 1) + [want[-1]]
        errors += S.check_locate(gpu, le, case, work, par, again, skip)[1]
    assert not errors, "\n".join(errors[:20])
