"""leoec_heal_dev / leoec_heal_rows: the host logic that needs no device.

leoec_heal_dev checks layout and parameters first (the statuses of
leoec_encode_dev), then k + m <= 32 (LEOEC_E_UNSUPPORTED), returns LEOEC_OK for
an empty batch, refuses bad pointers and strides (LEOEC_E_ARG) and only then
opens the device, so every status below is the same on a machine without one.

leoec_heal_rows gives, for one mask of lost ids, the survivors, the lost ids,
the coefficient rows and the mask's record in the device table.  For every
mask with 0..m bits the rows, applied on the host to the survivor blocks of
one oracle-encoded object, must give exactly the lost blocks, and the record
indices must be a bijection onto 0..N-1: a wrong rank or a wrong row here is
a wrong block on the device."""
import ctypes
import math

import numpy as np
import pytest

import heal_helpers as P

OK, E_NOT_ENOUGH, E_BAD_ID, E_UNSUPPORTED, E_ARG = 0, -9, -12, -14, -18
CID = {"cauchyrs": 1, "vandrs": 2, "liberation": 3, "isars": 4}

# (coding id, k, m, w): one of every parameter status of leoec_check_params
INVALID = [(0, 10, 4, 8), (7, 10, 4, 8), (2, 0, 4, 8), (2, 10, 0, 8), (2, 10, 4, 9),
           (2, 250, 10, 8), (1, 10, 4, 3), (1, 4, 2, 33), (3, 4, 3, 7), (3, 8, 2, 7),
           (3, 4, 2, 9), (3, 4, 2, 37), (4, 10, 4, 16), (4, 250, 10, 8)]
# valid parameters with more than 32 block ids, fused class and generic classes
WIDE = [(2, 29, 4, 8), (4, 30, 3, 8), (2, 20, 13, 16), (1, 28, 5, 8)]


class Bufs:
    """Host buffers standing in for device memory: no call below gets as far
    as the device, so nothing ever dereferences them."""

    def __init__(self):
        self.store = np.zeros(8192 + 64, dtype=np.uint8)
        self.p = (self.store.ctypes.data + 63) // 64 * 64  # 64-byte aligned
        self.q = self.p + 4096                             # a second, disjoint one


def _heal(le, cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, lost, unhealed):
    return le.lib.leoec_heal_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                                 lost, unhealed, None)


def test_heal_invalid_parameters_as_encode(le):
    """Invalid coding or parameters: the statuses of leoec_encode_dev, ahead
    of every other check (NULL pointers, aliased words, an empty batch)."""
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_encode_dev(coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, None)
        assert want < 0 and want == le.lib.leoec_check_params(coding, k, m, w)
        assert _heal(le, coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, b.p, b.q) == want
        assert _heal(le, coding, k, m, w, None, 0, 4096, 1, None, 0, None, None) == want
        assert _heal(le, coding, k, m, w, b.p, 4096, 4096, 0, b.p, 4096, b.p, b.p) == want


def test_heal_more_than_32_ids_unsupported(le):
    """k + m > 32 has no mask word: LEOEC_E_UNSUPPORTED, ahead of the empty
    batch and of the pointer checks."""
    b = Bufs()
    for coding, k, m, w in WIDE:
        assert le.lib.leoec_check_params(coding, k, m, w) == OK
        assert _heal(le, coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, b.p, b.q) == E_UNSUPPORTED
        assert _heal(le, coding, k, m, w, None, 0, 4096, 0, None, 0, None, None) == E_UNSUPPORTED
        assert _heal(le, coding, k, m, w, None, 0, 0, 3, None, 0, None, None) == E_UNSUPPORTED
        out = (ctypes.c_int * 40)()
        n = ctypes.c_int()
        assert le.lib.leoec_heal_rows(coding, k, m, w, 1, out, out, ctypes.byref(n), None, 0,
                                      None) == E_UNSUPPORTED
    # exactly 32 ids is served
    assert _heal(le, 2, 28, 4, 8, None, 0, 4096, 0, None, 0, None, None) == OK


def test_heal_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in [("vandrs", 10, 4, 8), ("cauchyrs", 10, 4, 8), ("liberation", 4, 2, 7)]:
        assert _heal(le, CID[cls], k, m, w, None, 0, 4096, 0, None, 0, None, None) == OK
        # an empty object has no blocks either
        assert _heal(le, CID[cls], k, m, w, None, 0, 0, 3, None, 0, None, None) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("cauchyrs", 10, 4, 8),
                                 ("vandrs", 6, 3, 32)], ids=str)
def test_heal_argument_errors(le, cfg):
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    p, q, ostr, pstr = b.p, b.q, 4096, m * bs
    for nobj in (1, 3):
        assert _heal(le, cid, k, m, w, None, ostr, size, nobj, p, pstr, p, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, None, pstr, p, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, None, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, p, None) == E_ARG
        # the two word arrays must not be one
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, q, q) == E_ARG
        # strides shorter than a row
        assert _heal(le, cid, k, m, w, p, size - 16, size, nobj, p, pstr, p, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr - 16, p, q) == E_ARG
        # misaligned buffers, words and strides
        assert _heal(le, cid, k, m, w, p + 8, ostr, size, nobj, p, pstr, p, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p + 8, pstr, p, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, p + 2, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, p, q + 2) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr + 8, size, nobj, p, pstr, p, q) == E_ARG
        assert _heal(le, cid, k, m, w, p, ostr, size, nobj, p, pstr + 8, p, q) == E_ARG


# ---------------------------------------------------------------------------
# leoec_heal_rows

def _one_object(le, oracle, cls, k, m, w):
    """One oracle-encoded object whose blocks hold two 16-byte columns (per
    packet, for the bitsliced classes), the last data block ragged."""
    size = k * w * 32 - 5
    bs, _ = le.layout(cls, (k, m, w), size)
    assert bs == 32 * w
    rng = np.random.Generator(np.random.PCG64(k * 131 + m * 17 + w))
    data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
    return [np.frombuffer(b, dtype=np.uint8) for b in oracle.encode(cls, k, m, w, data)]


def _check_rows(le, oracle, cfg, fused, count):
    cls, k, m, w = cfg
    blocks = _one_object(le, oracle, cls, k, m, w)
    masks = P.all_masks(k, m)
    assert len(masks) == count + 1 and masks[0] == 0
    seen = set()
    for mask in masks:
        surv, want, rows, index = le.device.heal_rows(cls, (k, m, w), mask)
        lost = P.ids_of(mask)
        assert want == lost, hex(mask)
        assert surv == [b for b in range(k + m) if b not in lost][:k], hex(mask)
        assert len(rows) == len(lost) and all(len(r) == k for r in rows)
        if fused and mask:
            assert 0 <= index < count, (hex(mask), index)
            seen.add(index)
        else:
            assert index == -1, (hex(mask), index)
        got = P.apply_rows(oracle, cls, w, rows, [blocks[s] for s in surv])
        for b, g in zip(lost, got):
            assert np.array_equal(g, blocks[b]), f"{cfg} mask {mask:#x}: block {b} from rows {rows}"
    if fused:
        assert seen == set(range(count))  # every record taken exactly once


@pytest.mark.parametrize("cfg,count", [(("vandrs", 10, 4, 8), 1470), (("vandrs", 4, 2, 8), 21),
                                       (("isars", 10, 4, 8), 1470), (("vandrs", 16, 4, 8), 6195)],
                         ids=str)
def test_heal_rows_fused(le, oracle, cfg, count):
    """Every mask with 0..m bits: the record indices of the non-zero ones are
    a bijection onto 0..N-1, the survivors are the first k intact ids, and
    the rows rebuild the lost blocks of an oracle-encoded object."""
    _check_rows(le, oracle, cfg, True, count)


def _rank(k, m, mask):
    """heal_table.hpp's record index, restated: first[p] + sum of C(b_i, i)
    over the set bits b_1 < ... < b_p, first[p] = sum of C(k + m, q), q < p."""
    ids = P.ids_of(mask)
    return (sum(math.comb(k + m, q) for q in range(1, len(ids))) +
            sum(math.comb(b, i) for i, b in enumerate(ids, 1)))


@pytest.mark.parametrize("cls", ["vandrs", "isars"])
def test_heal_rows_every_fused_configuration(le, oracle, cls):
    """k = 1..16 x m = 1..4, all 64 configurations of the class (one gf8_heal
    table each): every single-block mask and the cyclic runs of m blocks from
    every block.  The rows rebuild the lost 256-byte blocks of an
    oracle-encoded object, and the record index is the combinatorial rank.
    This pins the table contents of the configurations whose gf8_heal launch
    no device test runs (tests/gf8_heal_instances_child.py heals 32 of them)."""
    for k in range(1, 17):
        for m in range(1, 5):
            n = k + m
            blocks = _one_object(le, oracle, cls, k, m, 8)
            assert len(blocks[0]) == 256
            masks = [1 << b for b in range(n)]
            masks += [P.bits((b + x) % n for x in range(m)) for b in range(n)]
            for mask in dict.fromkeys(masks):
                surv, want, rows, index = le.device.heal_rows(cls, (k, m, 8), mask)
                lost = P.ids_of(mask)
                assert want == lost and len(rows) == len(lost), (cls, k, m, hex(mask))
                assert surv == [b for b in range(n) if b not in lost][:k], (cls, k, m, hex(mask))
                assert index == _rank(k, m, mask), (cls, k, m, hex(mask), index)
                got = P.apply_rows(oracle, cls, 8, rows, [blocks[s] for s in surv])
                for b, g in zip(lost, got):
                    assert np.array_equal(g, blocks[b]), f"{cls}({k},{m}) mask {mask:#x}: block {b}"


@pytest.mark.parametrize("cfg,count", [(("cauchyrs", 6, 3, 4), 9 + 36 + 84),
                                       (("vandrs", 6, 3, 32), 9 + 36 + 84)], ids=str)
def test_heal_rows_generic(le, oracle, cfg, count):
    """The same rows where no device table exists: index == -1."""
    _check_rows(le, oracle, cfg, False, count)


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("vandrs", 4, 2, 8), ("isars", 10, 4, 8),
                                 ("vandrs", 16, 4, 8), ("cauchyrs", 6, 3, 4), ("vandrs", 6, 3, 32)],
                         ids=str)
def test_heal_rows_errors(le, cfg):
    """Every mask with m + 1 bits: LEOEC_E_NOT_ENOUGH_BLOCKS; a bit at or above
    k + m: LEOEC_E_BAD_ID, also beside too many bits."""
    cls, k, m, w = cfg
    surv, want = (ctypes.c_int * k)(), (ctypes.c_int * 8)()
    n, idx = ctypes.c_int(), ctypes.c_int()

    def rc(mask):
        return le.lib.leoec_heal_rows(CID[cls], k, m, w, mask, surv, want, ctypes.byref(n), None, 0,
                                      ctypes.byref(idx))

    for mask in P.all_masks(k, m, m + 1, m + 1):
        assert rc(mask) == E_NOT_ENOUGH, hex(mask)
    high = [1 << b for b in range(k + m, 32)] + [1 | 1 << (k + m), 0xFFFFFFFF, 0x80000001,
                                                 (1 << (k + m + 1)) - 1]
    for mask in high:
        assert rc(mask) == E_BAD_ID, hex(mask)
    assert rc(P.bits(range(m))) == OK and n.value == m
    # the wrapper raises the same
    with pytest.raises(le.LeoecError) as e:
        le.device.heal_rows(cls, (k, m, w), (1 << (m + 1)) - 1)
    assert e.value.code == E_NOT_ENOUGH


def test_heal_rows_arguments(le):
    surv, want, n = (ctypes.c_int * 10)(), (ctypes.c_int * 4)(), ctypes.c_int()
    coef = (ctypes.c_uint32 * 40)()
    L = le.lib
    assert L.leoec_heal_rows(2, 10, 4, 8, 3, None, want, ctypes.byref(n), None, 0, None) == E_ARG
    assert L.leoec_heal_rows(2, 10, 4, 8, 3, surv, None, ctypes.byref(n), None, 0, None) == E_ARG
    assert L.leoec_heal_rows(2, 10, 4, 8, 3, surv, want, None, None, 0, None) == E_ARG
    assert L.leoec_heal_rows(2, 10, 4, 8, 3, surv, want, ctypes.byref(n), coef, 19, None) == E_ARG
    assert L.leoec_heal_rows(2, 10, 4, 8, 3, surv, want, ctypes.byref(n), coef, 20, None) == OK
    # liberation has survivors and lost ids but no GF(2^w) rows
    assert L.leoec_heal_rows(3, 4, 2, 7, 3, surv, want, ctypes.byref(n), None, 0, None) == OK
    assert (n.value, list(surv[:4]), list(want[:2])) == (2, [2, 3, 4, 5], [0, 1])
    assert L.leoec_heal_rows(3, 4, 2, 7, 3, surv, want, ctypes.byref(n), coef, 40, None) == E_UNSUPPORTED
    for coding, k, m, w in INVALID:
        assert L.leoec_heal_rows(coding, k, m, w, 1, surv, want, ctypes.byref(n), None, 0,
                                 None) == L.leoec_check_params(coding, k, m, w)
