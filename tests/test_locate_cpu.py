"""leoec_locate_dev / leoec_locate_rows: everything that needs no device.

leoec_locate_dev checks layout and parameters first (the statuses of
leoec_check_params), then whether it serves the configuration
(LEOEC_E_UNSUPPORTED), returns LEOEC_OK for an empty batch, refuses bad
pointers and strides (LEOEC_E_ARG) and only then opens the device, so every
status below is the same on a machine without one.

leoec_locate_rows gives the ratios T[i][j] = C[i][j] / C[0][j].  The host
model of locate_helpers applies them to the syndromes of oracle-encoded
blocks; here it must name every single damaged block, answer
LEOEC_LOCATE_MANY for two damaged blocks where m >= 3 (and that or a third
block where m = 2, the documented limit), and give the words
test_device_locate.py expects of the device for its damaged batches."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import gpu_helpers as H
import locate_helpers as L

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "leo_erasure_amd", "csrc")
OK, E_UNSUPPORTED, E_ARG = 0, -14, -18
CID = {"cauchyrs": 1, "vandrs": 2, "liberation": 3, "isars": 4}

# (coding id, k, m, w): one of every parameter status of leoec_check_params
INVALID = [(0, 10, 4, 8), (7, 10, 4, 8), (2, 0, 4, 8), (2, 10, 0, 8), (2, 10, 4, 9),
           (2, 250, 10, 8), (1, 10, 4, 3), (1, 4, 2, 33), (3, 4, 3, 7), (3, 8, 2, 7),
           (3, 4, 2, 9), (3, 4, 2, 37), (4, 10, 4, 16), (4, 250, 10, 8)]
# valid parameters leoec_locate_dev does not serve: each other class and
# width, then m = 1, k = 17 and m = 5 of both served classes
UNSERVED = [("cauchyrs", 10, 4, 8), ("cauchyrs", 6, 3, 4), ("liberation", 4, 2, 7),
            ("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32),
            ("vandrs", 10, 1, 8), ("isars", 10, 1, 8), ("vandrs", 17, 4, 8), ("isars", 17, 4, 8),
            ("vandrs", 10, 5, 8), ("isars", 10, 5, 8)]
SERVED = [("vandrs", 10, 4, 8), ("isars", 10, 4, 8), ("vandrs", 4, 2, 8), ("vandrs", 16, 4, 8),
          ("isars", 1, 2, 8)]


class Bufs:
    """Host buffers standing in for device memory: no call below gets as far
    as the device, so nothing ever dereferences them."""

    def __init__(self):
        self.store = np.zeros(4096 + 64, dtype=np.uint8)
        self.p = (self.store.ctypes.data + 63) // 64 * 64  # 64-byte aligned


def _locate(le, cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, lost):
    return le.lib.leoec_locate_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity,
                                   parity_stride, lost, None)


def _rows_rc(le, cid, k, m, w, cap=None):
    cap = (m - 1) * k if cap is None else cap
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_locate_rows(cid, k, m, w, out, cap), list(out)


def test_helpers_agree_with_the_header(le):
    assert L.MANY == le.device.LOCATE_MANY == 0x80000000
    for cfg in SERVED:
        assert L.served(*cfg)
    for cfg in UNSERVED:
        assert not L.served(*cfg)
    assert all(L.served(*f[:4]) for f in L.FAMILIES)
    # the bit lies above every id of a served configuration
    assert L.MANY >> (16 + 4) != 0


def test_locate_invalid_parameters_as_check_params(le):
    """Invalid coding or parameters: leoec_check_params' status, ahead of
    every other check (NULL pointers, an empty batch), from both calls."""
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_check_params(coding, k, m, w)
        assert want < 0
        assert _locate(le, coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, b.p) == want
        assert _locate(le, coding, k, m, w, None, 0, 4096, 1, None, 0, None) == want
        assert _locate(le, coding, k, m, w, None, 0, 4096, 0, None, 0, None) == want
        assert _rows_rc(le, coding, k, m, w, 64)[0] == want
        assert le.lib.leoec_locate_rows(coding, k, m, w, None, 0) == want


@pytest.mark.parametrize("cfg", UNSERVED, ids=str)
def test_locate_unserved_configurations(le, cfg):
    """LEOEC_E_UNSUPPORTED without a device, ahead of the pointer checks and
    of the empty batch, from both calls."""
    cls, k, m, w = cfg
    cid = CID[cls]
    assert le.lib.leoec_check_params(cid, k, m, w) == OK
    b = Bufs()
    bs, _ = le.layout(cls, (k, m, w), 4000)
    assert _locate(le, cid, k, m, w, b.p, 4096, 4000, 1, b.p, m * bs, b.p) == E_UNSUPPORTED
    assert _locate(le, cid, k, m, w, None, 0, 4000, 1, None, 0, None) == E_UNSUPPORTED
    assert _locate(le, cid, k, m, w, None, 0, 4000, 0, None, 0, None) == E_UNSUPPORTED
    assert _rows_rc(le, cid, k, m, w, 256)[0] == E_UNSUPPORTED
    assert le.lib.leoec_locate_rows(cid, k, m, w, None, 0) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.locate_rows(cls, (k, m, w))
    assert e.value.code == E_UNSUPPORTED


def test_locate_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in SERVED:
        assert _locate(le, CID[cls], k, m, w, None, 0, 4096, 0, None, 0, None) == OK
        # an empty object has no blocks either
        assert _locate(le, CID[cls], k, m, w, None, 0, 0, 3, None, 0, None) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("isars", 10, 4, 8), ("vandrs", 4, 2, 8)],
                         ids=str)
def test_locate_argument_errors(le, cfg):
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    p, ostr, pstr = b.p, 4096, m * bs
    for nobj in (1, 3):
        assert _locate(le, cid, k, m, w, None, ostr, size, nobj, p, pstr, p) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr, size, nobj, None, pstr, p) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, None) == E_ARG
        # strides shorter than a row
        assert _locate(le, cid, k, m, w, p, size - 16, size, nobj, p, pstr, p) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr, size, nobj, p, pstr - 16, p) == E_ARG
        # misaligned buffers, words and strides
        assert _locate(le, cid, k, m, w, p + 8, ostr, size, nobj, p, pstr, p) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr, size, nobj, p + 8, pstr, p) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, p + 2) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr + 8, size, nobj, p, pstr, p) == E_ARG
        assert _locate(le, cid, k, m, w, p, ostr, size, nobj, p, pstr + 8, p) == E_ARG


# ---------------------------------------------------------------------------
# leoec_locate_rows

def _matrix(le, cid, k, m, w):
    out, n = (ctypes.c_uint32 * (m * k))(), ctypes.c_int()
    assert le.lib.leoec_coding_matrix(cid, k, m, w, out, m * k, ctypes.byref(n)) == OK
    assert n.value == m * k
    return [list(out[i * k:(i + 1) * k]) for i in range(m)]


def _check_ratio(le, oracle, cls, k, m):
    C = _matrix(le, CID[cls], k, m, 8)
    T = le.device.locate_rows(cls, (k, m, 8))
    assert len(T) == m - 1 and all(len(r) == k for r in T)
    for i in range(1, m):
        for j in range(k):
            assert C[0][j] != 0 and C[i][j] != 0
            assert T[i - 1][j] == oracle.gf_div(C[i][j], C[0][j], 8), (cls, k, m, i, j)
            assert oracle.gf_mul(T[i - 1][j], C[0][j], 8) == C[i][j]


def test_locate_rows_are_the_matrix_ratios(le, oracle):
    """T[i][j] == C[i][j] / C[0][j] of leoec_coding_matrix, division and
    product from the oracle: every family, and k = 1..16 x m = 2..4 of both
    classes (none of the 96 is refused for a zero entry or a singular minor)."""
    for cls, k, m, w, B in L.FAMILIES:
        _check_ratio(le, oracle, cls, k, m)
    for cls in ("vandrs", "isars"):
        for k in range(1, 17):
            for m in range(2, 5):
                _check_ratio(le, oracle, cls, k, m)


def test_locate_rows_arguments(le):
    for cls, k, m, w in SERVED:
        need = (m - 1) * k
        assert _rows_rc(le, CID[cls], k, m, w, need)[0] == OK
        assert _rows_rc(le, CID[cls], k, m, w, need - 1)[0] == E_ARG
        assert le.lib.leoec_locate_rows(CID[cls], k, m, w, None, need) == E_ARG
        # a larger buffer is filled up to (m-1) k words and no further
        rc, out = _rows_rc(le, CID[cls], k, m, w, need + 3)
        assert rc == OK and out[need:] == [0, 0, 0] and all(out[:need])


def test_builder_refuses_what_it_cannot_name(le, oracle, tmp_path):
    """locate_build_rows itself (plain C++, built here without HIP): a matrix
    with a zero entry or a singular 2 x 2 minor is LEOEC_E_UNSUPPORTED, as is
    m = 1; the (10,4) vandrs matrix with one entry changed either way is
    refused, unchanged it gives leoec_locate_rows' words."""
    so = str(tmp_path / "liblocate_rows_test.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall",
                    os.path.join(HERE, "locate_rows_test.cpp"),
                    os.path.join(CSRC, "locate_rows.cpp"), os.path.join(CSRC, "codes.cpp"),
                    "-o", so], check=True)
    B = ctypes.CDLL(so)

    def build(C, k, m):
        flat = (ctypes.c_uint32 * (m * k))(*[x for row in C for x in row])
        out = (ctypes.c_uint32 * max((m - 1) * k, 1))()
        return B.locate_rows_of(flat, k, m, out), list(out)

    assert build([[1, 2], [1, 3]], 2, 2) == (OK, [1, oracle.gf_div(3, 2, 8)])
    assert build([[1, 0], [1, 3]], 2, 2)[0] == E_UNSUPPORTED   # a zero entry
    assert build([[1, 2], [0, 3]], 2, 2)[0] == E_UNSUPPORTED
    assert build([[1, 2], [2, 4]], 2, 2)[0] == E_UNSUPPORTED   # rows in proportion
    assert build([[1, 2]], 2, 1)[0] == E_UNSUPPORTED           # one coding block
    C = _matrix(le, CID["vandrs"], 10, 4, 8)
    rc, T = build(C, 10, 4)
    assert rc == OK and [T[i * 10:(i + 1) * 10] for i in range(3)] == \
        le.device.locate_rows("vandrs", (10, 4, 8))
    zero = [row[:] for row in C]
    zero[2][7] = 0
    assert build(zero, 10, 4)[0] == E_UNSUPPORTED
    # rows 1, 3 and columns 4, 9: make the minor singular by solving for one entry
    sing = [row[:] for row in C]
    sing[3][9] = oracle.gf_div(oracle.gf_mul(C[1][9], C[3][4], 8), C[1][4], 8)
    assert sing[3][9] not in (0, C[3][9])
    assert build(sing, 10, 4)[0] == E_UNSUPPORTED


# ---------------------------------------------------------------------------
# The host model

@pytest.fixture(scope="module", params=L.FAMILIES, ids=L.family_id)
def family(request):
    return request.param


def _model_cases(le, oracle, family):
    """The family at its whole-block size and at edge_sizes' one-byte object
    (one object each)."""
    cls, k, m, w, B = family
    sizes = H.edge_sizes(k, w, B)
    assert sizes[0] == k * B and sizes[-1] == 1
    return [H.edge_case(le, oracle, family[:4], size, n=1) for size in (sizes[0], sizes[-1])]


def _valid(case, b):
    """Valid bytes of block b."""
    return case.bs if b >= case.k else H.block_valids(case.k, case.bs, case.size)[b]


def _hit(case, b, col, x):
    """One damage entry: byte `col` of block b of object 0."""
    if b < case.k:
        return ("objs", 0, b * case.bs + col, x)
    return ("parity", 0, (b - case.k) * case.bs + col, x)


def test_model_names_every_single_block(le, oracle, family):
    """Each block with a valid byte damaged in turn, in one byte and then in
    every valid byte: the model names it."""
    cls, k, m, w, B = family
    for case in _model_cases(le, oracle, family):
        assert L.model_words(oracle, le, case, []) == [0]
        rng = np.random.Generator(np.random.PCG64(case.size + k))
        for b in range(k + m):
            v = _valid(case, b)
            if v == 0:
                continue
            one = [_hit(case, b, (b * 977) % v, L.BIT)]
            assert L.model_words(oracle, le, case, one) == [1 << b], (case.ident(), b, one)
            whole = [_hit(case, b, c, int(x)) for c, x in enumerate(rng.integers(1, 256, v))]
            assert L.model_words(oracle, le, case, whole) == [1 << b], (case.ident(), b, "whole")


def test_model_two_damaged_blocks(le, oracle, family):
    """Every pair of blocks damaged in one byte column.  m >= 3:
    LEOEC_LOCATE_MANY, always.  m = 2 (the documented limit): that, or one
    block that is neither of the two."""
    cls, k, m, w, B = family
    for case in _model_cases(le, oracle, family):
        ids = [b for b in range(k + m) if _valid(case, b)]
        rng = np.random.Generator(np.random.PCG64(case.size + m))
        for a, b in itertools.combinations(ids, 2):
            col = int(rng.integers(0, min(_valid(case, a), _valid(case, b))))
            xa, xb = (int(x) for x in rng.integers(1, 256, 2))
            got = L.model_words(oracle, le, case, [_hit(case, a, col, xa), _hit(case, b, col, xb)])[0]
            if m >= 3:
                assert got == L.MANY, (case.ident(), a, b, hex(got))
            else:
                third = [1 << c for c in range(k + m) if c not in (a, b)]
                assert got == L.MANY or got in third, (case.ident(), a, b, hex(got))


def test_model_gives_the_device_tests_words(le, oracle, family):
    """No GPU: for every case of test_device_locate.py the model gives the
    words that test expects of the device, and the damage lies inside valid
    bytes (model_words asserts that)."""
    cls, k, m, w, B = family
    for size in H.edge_sizes(k, w, B):
        case = H.edge_case(le, oracle, family[:4], size)
        for dmg, want in L.expected_calls(case):
            assert len({(wh, o, p) for wh, o, p, _ in dmg}) == len(dmg)
            assert L.model_words(oracle, le, case, dmg) == want, (case.ident(), want)
