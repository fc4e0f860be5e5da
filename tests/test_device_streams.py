"""The device calls off the null stream: captured into a graph and replayed,
and as a scrub pipeline on a side stream (stream_helpers.py has the why and
the harness).

include/leoec.h promises that the work of every device call is enqueued on
`stream` and that the call returns without synchronising.  Every other module
passes the null stream, where a memset or a launch that took stream 0, one
launch of a multi-launch plan on another stream, a hidden allocation or a
blocking copy changes nothing that a test can see.

Families: verify_helpers.FAMILIES, 15 rows, which between them reach every
launch shape: one gf8_apply and its 64-lane form (B = 164,992), the K > 16
accumulating chain (vandrs(20,4,8)), two row groups (vandrs(6,5,8)),
gfbit_apply, the generic bit kernel (cauchyrs(5,3,17)), the liberation encode
and syndrome kernels, gfs_apply at w = 16 and 32.  One size per family,
k B - 17: a ragged last block and a partial last tile.

  captured   encode, decode (two erasure sets), repair, verify (fused: no
             workspace; two-pass: 2 m bs bytes, three chunks) over EDGE_N = 5
             objects; heal over the five fused rows and 9 objects.  Every
             capture is one call on one stream: no forks, no events.  The
             generic heal synchronises and is never captured.
  pipeline   fill, copies, verify, locate_gfw, heal, verify on a non-blocking
             side stream over heal_helpers.RUN_N = 12 objects whose damaged
             blocks form run_masks' runs: the non-fused rows heal through
             heal_generic, with runs, off the null stream.

The captured heal wants the code's pattern table cached (at most 16 per
process, heal.hip); the four fused codes here are among the first the suite
heals, in test_device_heal.py."""
import pytest

import gpu_helpers as H
import heal_helpers as P
import locate_gfw_helpers as G
import locate_helpers as L
import scrub_helpers as S
import stream_helpers as T
import verify_helpers as V


@pytest.fixture(scope="module", params=T.FAMILIES, ids=T.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once)"""
    return request.param


def _case(le, oracle, family, n=H.EDGE_N):
    return H.edge_case(le, oracle, family[:4], T.edge_size(family), n=n)


# ---------------------------------------------------------------------------
# No GPU: the inputs of the tests below.

def test_families_and_sizes():
    """15 rows, five of them fused; k B - 17 leaves every block with valid
    bytes, the last one ragged by 17."""
    assert len(T.FAMILIES) == 15 and len(set(T.FAMILIES)) == 15
    assert [f for f in T.FAMILIES if P.fused(*f[:4])] == T.HEAL_FAMILIES and len(T.HEAL_FAMILIES) == 5
    for cls, k, m, w, B in T.FAMILIES:
        assert T.edge_size((cls, k, m, w, B)) == k * B - 17
        assert G.served(cls, k, m, w)  # locate_gfw answers for every row


def test_rotated_batch_differs_everywhere(le, oracle, family):
    """No GPU: object o of the rotated batch holds object (o + 1) mod n, and
    every one of its blocks, the m coding blocks included, differs from the
    block the original batch has there: a replay that read stale inputs or
    left stale outputs is wrong in every object."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family)
    assert case.bs == B and H.block_valids(k, case.bs, case.size)[-1] == B - 17
    rot = T.rotation(case.n)
    assert sorted(rot) == list(range(case.n)) and all(rot[o] != o for o in range(case.n))
    for o in range(case.n):
        for b in range(k + m):
            assert (case.blocks[b, o] != case.blocks[b, rot[o]]).any(), (o, b)


def test_erasures_and_repairs(family):
    """No GPU: both erasure sets of the captured decode lose m blocks, a data
    block among them; the repaired pair is the last data block and the first
    coding block."""
    cls, k, m, w, B = family
    sets = H.edge_erasures(k, m)[:2]
    assert sets[0] == list(range(k - m, k))
    assert sets[1] == sorted(([0, k - 1] + list(range(k, k + m)))[:m])
    assert all(len(s) == m and min(s) < k for s in sets)
    assert H.edge_repairs(k, m)[0] == [k - 1, k]


def test_verify_batches_from_oracle(le, oracle, family):
    """No GPU: the words the captured verify must give are the oracle's: the
    damaged data re-encoded and the damaged coding blocks compared with it."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family)
    batches = T.verify_batches(oracle, case)
    assert [want for _, want in batches] == [[1, 1 << (m - 1), (1 << m) - 1, 0, 0]] * 2 + [[0] * 5]
    for dmg, want in batches:
        assert S.oracle_flags(oracle, case, L.with_bit(dmg)) == want


def test_workspace_gives_three_chunks(le, oracle, family):
    """No GPU: the two-pass families' captured verify gets 2 m bs bytes where
    the query wants 5 m bs: chunks of 2, 2 and 1 objects; the fused families
    need none."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family)
    need = le.device.verify_workspace(cls, case.params, case.size, case.n)
    nbytes = T.verify_workspace_bytes(case)
    if V.fused(cls, k, m, w):
        assert need == 0 and nbytes is None
    else:
        assert need == case.n * m * case.bs and nbytes == 2 * m * case.bs
        assert T.ws_chunks(case.n, nbytes, m, case.bs) == [(0, 2), (2, 2), (4, 1)]


def test_heal_masks_reversed():
    """No GPU: reversing edge_masks changes the mask of every object but the
    middle one, and moves the unrecoverable masks to the front."""
    for cls, k, m, w, B in T.HEAL_FAMILIES:
        masks = P.edge_masks(k, m)
        rev = masks[::-1]
        assert [o for o in range(P.EDGE_N) if masks[o] == rev[o]] == [P.EDGE_N // 2]
        assert [P.recoverable(x, k, m) for x in rev] == [False] * 2 + [True] * 7


def test_pipeline_damage(le, oracle, family):
    """No GPU: the pipeline's batch has run_masks' runs; every damaged block
    takes its 64 hits inside valid bytes (damaged_objects asserts it); the
    first flags are the oracle's and the located words the host model's."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family, n=P.RUN_N)
    blocks = T.run_blocks(k, m)
    assert [r[2] for r in P.runs_of(blocks)] == [r[2] for r in P.runs_of(P.run_masks(k, m))] == \
        [3, 2, 2, 2, 1, 2]
    dmg, verify, locate = T.pipeline_damage(case, blocks)
    assert len(dmg) == S.HITS * sum(b is not None for b in blocks)
    assert locate == [0 if b is None else 1 << b for b in blocks]
    assert [r[2] for r in P.runs_of(locate)] == [3, 2, 2, 2, 1, 2]  # what heal_generic groups
    assert all(P.recoverable(x, k, m) for x in locate)
    assert S.oracle_flags(oracle, case, dmg) == verify
    if G.word_class(cls, k, m, w):
        model = G.model_words(oracle, le, case, dmg)
    else:
        model = [x for _, x in sorted(S.model_words(oracle, le, case, dmg).items())]
    assert model == locate


# ---------------------------------------------------------------------------
# Captured and replayed.

@pytest.mark.gpu
def test_device_encode_captured(gpu, le, oracle, family):
    """Nothing runs during the capture (parity keeps its 0x5A); three replays
    give the oracle's coding blocks of the batch, of the rotated batch and of
    the batch again, every other byte of both arenas unchanged."""
    errors = T.captured_encode(gpu, le, _case(le, oracle, family))
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_decode_captured(gpu, le, oracle, family):
    """One graph per erasure set (the last m data blocks; {0, k-1} plus coding
    blocks): the poison survives the capture, and every replay rebuilds the
    erased data blocks of the batch then in the buffers."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family)
    errors = []
    for erased in H.edge_erasures(k, m)[:2]:
        errors += T.captured_decode(gpu, le, case, erased)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_repair_captured(gpu, le, oracle, family):
    """The last data block and the first coding block from every other block:
    the outputs keep their 0x3C through the capture, and every replay gives
    the oracle's blocks of the batch then in the buffers."""
    cls, k, m, w, B = family
    errors = T.captured_repair(gpu, le, _case(le, oracle, family), H.edge_repairs(k, m)[0])
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_verify_captured(gpu, le, oracle, family):
    """Flags keep their 0xFFFFFFFF and the workspace its 0xEE through the
    capture; the replays give the words of both damaged batches and zeros for
    the clean one.  Two-pass families: memset, then three encode and compare
    chunks that reuse the same workspace rows, all in the graph."""
    errors = T.captured_verify(gpu, le, oracle, _case(le, oracle, family))
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("family", T.HEAL_FAMILIES, ids=T.family_id)
def test_device_heal_captured(gpu, le, oracle, family):
    """The fused path, 9 objects, edge_masks: the poison and the unhealed
    pre-fill survive the capture; `lost` is rewritten between the replays (the
    masks, reversed, the masks) and every replay heals what its masks name."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family, n=P.EDGE_N)
    errors = T.captured_heal(gpu, le, case, P.edge_masks(k, m))
    assert not errors, "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# The scrub pipeline on a side stream.

@pytest.mark.gpu
def test_device_scrub_pipeline_on_side_stream(gpu, le, oracle, family):
    """A 512 MiB fill, the copies of the damaged batch, verify, locate_gfw,
    heal and verify on a non-blocking stream, then that stream's
    synchronisation alone: flags and words of the damage, both arenas back to
    the snapshots byte for byte, unhealed and the second flags 0."""
    cls, k, m, w, B = family
    case = _case(le, oracle, family, n=P.RUN_N)
    errors = T.run_pipeline(gpu, le, case, T.run_blocks(k, m))
    assert not errors, "\n".join(errors[:20])
