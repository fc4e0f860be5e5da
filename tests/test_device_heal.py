"""leoec_heal_dev on the device: per-object lost blocks rebuilt in place,
bit-exact, on the edge harness of gpu_helpers (guarded arenas, random non-zero
bytes behind every object, every byte of both arenas compared afterwards).

Cases: every family of gpu_helpers.EDGE_FAMILIES at every size of edge_sizes
(whole tiles, a partial last tile, a ragged last block, empty trailing
blocks; the 164,992-byte vandrs row is gf8_heal's 64-lane form) plus
vandrs(20,4,8) and vandrs(6,5,8), the GF(2^8) shapes outside one gf8_heal
launch.  Which path serves which row (heal.hip):

  vandrs(10,4,8), (4,2,8), (7,3,8), isars(10,4,8)   gf8_heal, one launch
  everything else                                   masks copied back, one
                                                    plan launch per run

Every batch has heal_helpers.EDGE_N = 9 objects, one per mask of
heal_helpers.edge_masks: clean, six recoverable patterns (data and coding
blocks, ragged and empty outputs) and two unrecoverable ones.  All
expectations are the oracle's blocks (the snapshots of the EdgeCase)."""
import pytest

import gpu_helpers as H
import heal_helpers as P


@pytest.fixture(scope="module", params=P.FAMILIES, ids=P.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def _cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in H.edge_sizes(k, w, B):
        yield H.edge_case(le, oracle, family[:4], size, n=P.EDGE_N)


def test_edge_masks_are_what_they_claim():
    """No GPU: the mask list of every family, spelled out."""
    for cls, k, m, w, B in P.FAMILIES:
        masks = P.edge_masks(k, m)
        assert len(masks) == P.EDGE_N and k > m >= 2
        ids = [P.ids_of(x) for x in masks]
        assert ids[0] == []
        assert ids[1] == list(range(k - m, k))
        assert ids[2] == sorted(([0, k - 1] + list(range(k, k + m)))[:m]) and len(ids[2]) == m
        assert ids[3] == [k - 1]
        assert ids[4] == list(range(m))
        assert ids[5] == list(range(k, k + m))
        assert ids[6] == [k + m - 1]
        assert len(ids[7]) == m + 1 and max(ids[7]) < k + m
        assert ids[8] == [0, k + m]
        assert [P.recoverable(x, k, m) for x in masks] == [True] * 7 + [False] * 2
        assert len(set(masks)) == P.EDGE_N  # no run of equal masks: one launch each on the generic path
    assert sum(P.fused(*f[:4]) for f in P.FAMILIES) == 5  # the 64-lane row included
    assert all(P.fused(*f[:4]) for f in P.GF8_FAMILIES)


@pytest.mark.gpu
def test_device_heal_edges(gpu, le, oracle, family):
    """Healed rows equal the snapshots, unrecoverable rows keep their poison,
    guard rows and bytes past `size` are unchanged, unhealed is
    [0, ..., mask, mask] between intact sentinels, lost is unchanged."""
    cls, k, m, w, B = family
    errors = []
    for case in _cases(le, oracle, family):
        errors += P.run_heal(gpu, le, case, P.edge_masks(k, m))
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_heal_partial_batch(gpu, le, oracle, family):
    """nobj = n - 2 with the two unrecoverable masks moved to the front: the
    rows and words of the last two objects (both damaged, both recoverable)
    keep their pre-fill."""
    cls, k, m, w, B = family
    em = P.edge_masks(k, m)
    masks = em[7:] + em[:7]
    errors = []
    for case in _cases(le, oracle, family):
        errors += P.run_heal(gpu, le, case, masks, nobj=case.n - 2)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,size,count", [(("vandrs", 10, 4, 8), 1277, 1471),
                                            (("vandrs", 4, 2, 8), 509, 22)], ids=str)
def test_device_heal_every_pattern(gpu, le, oracle, cfg, size, count):
    """Every mask of 0..m bits once in one batch, then 8 unrecoverable masks:
    a wrong rank or a wrong record is a wrong block here.  bs 128, the last
    data block 125 bytes."""
    cls, k, m, w = cfg
    masks = P.all_masks(k, m) + P.unrecoverable_masks(k, m)
    assert len(masks) == count + 8 and not any(P.recoverable(x, k, m) for x in masks[count:])
    case = H.EdgeCase(le, oracle, cfg, size, len(masks))
    assert case.bs == 128 and size - (k - 1) * case.bs == 125
    errors = P.run_heal(gpu, le, case, masks)
    assert not errors, "\n".join(errors[:20])
