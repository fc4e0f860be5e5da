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

The edge batches have heal_helpers.EDGE_N = 9 objects, one per mask of
heal_helpers.edge_masks: clean, six recoverable patterns (data and coding
blocks, ragged and empty outputs) and two unrecoverable ones.  No two of those
masks are equal, so on the generic path every damaged object is a run of its
own: one launch each, no > 1 never reached.  The run batches have
heal_helpers.RUN_N = 12 objects with heal_helpers.run_masks: runs of two and
three equal masks (one launch over several objects at a base offset of
first * stride), a clean run, an unrecoverable run, a run whose only lost block
lies past `size` at the small sizes (nothing to launch, unhealed still 0), and
a run cut by nobj.  All expectations are the oracle's blocks (the snapshots of
the EdgeCase)."""
import pytest

import gpu_helpers as H
import heal_helpers as P


@pytest.fixture(scope="module", params=P.FAMILIES, ids=P.family_id)
def family(request):
    """(module scope: the tests of one family run together and share its
    EdgeCases, the oracle's blocks computed once per size)"""
    return request.param


def _cases(le, oracle, family, n=P.EDGE_N):
    cls, k, m, w, B = family
    for size in H.edge_sizes(k, w, B):
        yield H.edge_case(le, oracle, family[:4], size, n=n)


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


def test_run_masks_are_what_they_claim(le):
    """No GPU: the run list of every family, spelled out: a run at the front
    and one at the back, a clean run, an unrecoverable run, every run abutting
    the next; and at the two smallest sizes block k-1 holds no byte below
    `size`, so the runs of {k-1} have nothing to write."""
    for cls, k, m, w, B in P.FAMILIES:
        masks = P.run_masks(k, m)
        assert len(masks) == P.RUN_N == 12
        a, b, c, U = masks[0], masks[5], masks[9], masks[7]
        assert masks == [a, a, a, 0, 0, b, b, U, U, c, a, a]
        assert P.ids_of(a) == [k - 1]
        assert P.ids_of(b) == sorted(([0, k - 1] + list(range(k, k + m)))[:m]) and len(P.ids_of(b)) == m
        assert P.ids_of(c) == list(range(k, k + m))
        assert P.ids_of(U) == list(range(k - 1, k + m))
        assert [P.recoverable(x, k, m) for x in (a, 0, b, U, c)] == [True, True, True, False, True]
        assert P.runs_of(masks) == [(a, 0, 3), (0, 3, 2), (b, 5, 2), (U, 7, 2), (c, 9, 1), (a, 10, 2)]
        assert len({a, 0, b, U, c}) == 5
        # nobj = RUN_N - 1 cuts the last run: object 10 alone is healed
        assert P.runs_of(masks[:P.RUN_N - 1])[-1] == (a, 10, 1)
        sizes = H.edge_sizes(k, w, B)
        for size in sorted(sizes)[:2]:
            bs, _ = le.layout(cls, (k, m, w), size)
            assert H.block_valids(k, bs, size)[k - 1] == 0 and (k - 1) * bs >= size
        assert H.block_valids(k, B, sizes[0])[k - 1] == B  # and at the large sizes it has bytes


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
def test_device_heal_runs(gpu, le, oracle, family):
    """run_masks over 12 objects at every size: the generic path's runs of
    two and three objects go out as one launch each, at first * stride; the
    clean and the unrecoverable run launch nothing; at the small sizes {k-1}
    is an empty block, its runs launch nothing and unhealed is 0 all the
    same.  (The fused rows take gf8_heal: the same batch, one launch.)"""
    cls, k, m, w, B = family
    errors = []
    for case in _cases(le, oracle, family, n=P.RUN_N):
        errors += P.run_heal(gpu, le, case, P.run_masks(k, m))
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
def test_device_heal_runs_cut_by_nobj(gpu, le, oracle, family):
    """nobj = 11: the last run is cut in two; object 10 is healed, object 11
    keeps its poison and its word its pre-fill."""
    cls, k, m, w, B = family
    errors = []
    for case in _cases(le, oracle, family, n=P.RUN_N):
        errors += P.run_heal(gpu, le, case, P.run_masks(k, m), nobj=P.RUN_N - 1)
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
