"""scrub_helpers' whole-block batch on the host (no GPU): for every case the
whole-block GPU tests of test_device_scrub.py, test_device_scrub_ws.py and the
two forms modules run, the damage lies inside valid bytes and covers every one
of the block's, the oracle's re-encoding gives the by-construction verify flags
and the host models (locate_helpers.model_word, locate_ws_helpers.model_word)
the by-construction words, 1 << b.  The only objects that expect 0 besides the
clean one are data blocks wholly past `size`: none at k B - 1, at most one at
the small size."""
import numpy as np
import pytest

import gpu_helpers as H
import locate_helpers as L
import locate_ws_helpers as W
import scrub_dev_helpers as D
import scrub_helpers as S

FAMILIES = L.FAMILIES + W.FAMILIES


def sizes(family):
    """scrub_dev_helpers.SCRUB.sizes for the fused families, SCRUB_WS.sizes'
    three for the bitmatrix ones."""
    return (D.SCRUB_WS if S.bitsliced(family[0]) else D.SCRUB).sizes(family)


def whole_cases(le, oracle, family):
    cls, k, m, w, B = family
    for size in sizes(family):
        yield H.edge_case(le, oracle, family[:4], size, n=k + m + 1)


def check_case(le, oracle, case, empty_allowed):
    """The assertions of one case; `empty_allowed`: data blocks that may lie
    wholly past `size`."""
    k, m = case.k, case.m
    blocks = S.whole_batch(case)
    assert blocks == list(range(k + m)) + [None]
    words = S.whole_words(case, blocks)
    empty = [b for b in range(k + m) if words[b] == 0]
    assert len(empty) <= empty_allowed and all(b < k and S.block_valid(case, b) == 0 for b in empty), \
        (case.ident(), empty)
    assert words == [0 if b in empty else 1 << b for b in range(k + m)] + [0]
    objs = S.whole_objects(case, blocks)  # asserts the damage inside valid bytes
    assert sorted(objs) == [b for b in range(k + m) if b not in empty]
    for b, (data, stored) in objs.items():
        clean, clean_stored = L.object_blocks(case, b)
        where, lo, hi = S.whole_span(case, b)
        assert hi - lo == S.block_valid(case, b)
        if where == "objs":
            diff = data != clean
            assert all(np.array_equal(x, y) for x, y in zip(stored, clean_stored))
        else:
            diff = np.concatenate(stored) != np.concatenate(clean_stored)
            assert np.array_equal(data, clean)
        # every valid byte of the block and no other
        assert diff[lo:hi].all() and int(diff.sum()) == hi - lo, (case.ident(), b)
    every = (1 << m) - 1
    flags = [0 if b in empty else every if b < k else 1 << (b - k) for b in range(k + m)] + [0]
    assert S.flags_of(oracle, case, objs) == flags, case.ident()
    model = S.words_of(oracle, le, case, objs)
    assert [model[o] for o in range(case.n)] == words, case.ident()


@pytest.mark.parametrize("family", FAMILIES, ids=L.family_id)
def test_whole_batch_against_oracle_and_model(le, oracle, family):
    cls, k, m, w, B = family
    assert W.served(cls, k, m, w)
    szs = sizes(family)
    assert szs[:2] == [k * B - 1, 16 * w * (k - 2) + 5]
    for case in whole_cases(le, oracle, family):
        # 16 w (k - 2) + 5: data block k - 1 is empty, block k - 2 has 5 bytes
        check_case(le, oracle, case, 1 if case.size == szs[1] else 0)


def test_dense_batch_blocks(le, oracle):
    """The dense variant: object o has block o mod (k + m) damaged, different
    values in objects that share a block."""
    case = H.EdgeCase(le, oracle, ("vandrs", 4, 2, 8), 4 * 4224 - 1, 15)
    blocks = S.whole_dense_batch(case)
    assert blocks == [o % 6 for o in range(15)]
    assert S.whole_words(case, blocks) == [1 << (o % 6) for o in range(15)]
    values = S.whole_values(case, blocks)
    assert [values[b][0] for b in range(6)] == [[o for o in range(15) if o % 6 == b] for b in range(6)]
    assert values[3][1].shape == (2, 4223) and values[0][1].shape == (3, 4224)
    assert not np.array_equal(values[0][1][0], values[0][1][1])
    objs = S.whole_objects(case, blocks)
    assert sorted(objs) == list(range(15))
    assert [S.words_of(oracle, le, case, objs)[o] for o in range(15)] == S.whole_words(case, blocks)
