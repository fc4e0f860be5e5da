"""leoec_locate_ws_dev / leoec_locate_ws_dev_workspace / leoec_locate_bitrows:
everything that needs no device.

leoec_locate_ws_dev checks layout and parameters first (the statuses of
leoec_check_params), then whether it serves the configuration
(LEOEC_E_UNSUPPORTED), returns LEOEC_OK for an empty batch, refuses bad
pointers, strides and workspaces (LEOEC_E_ARG) and only then opens the device,
so every status below is the same on a machine without one.

leoec_locate_bitrows gives the GF(2) ratios T[i][j] = B[i][j] B[0][j]^-1.  A
numpy model built from the oracle's bitmatrices checks them by matrix product
mod 2; the host model of locate_ws_helpers applies them to the syndrome
packets of oracle-encoded blocks and must give the words
test_device_locate_ws.py expects of the device (locate_helpers.expected_calls,
unchanged)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gpu_helpers as H
import locate_helpers as L
import locate_ws_helpers as W

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "leo_erasure_amd", "csrc")
OK, E_BAD_SIZE, E_UNSUPPORTED, E_ARG = 0, -13, -14, -18
CID = {"cauchyrs": 1, "vandrs": 2, "liberation": 3, "isars": 4}

# (coding id, k, m, w): one of every parameter status of leoec_check_params
INVALID = [(0, 10, 4, 8), (7, 10, 4, 8), (2, 0, 4, 8), (2, 10, 0, 8), (2, 10, 4, 9),
           (2, 250, 10, 8), (1, 10, 4, 3), (1, 4, 2, 33), (3, 4, 3, 7), (3, 8, 2, 7),
           (3, 4, 2, 9), (3, 4, 2, 37), (4, 10, 4, 16), (4, 250, 10, 8)]
# valid parameters leoec_locate_ws_dev does not serve: vandrs w = 16 / 32,
# w = 8 with m = 1, k > 16 or m > 4, bitmatrix m = 1, k + m > 32, a table
# above 768 words
UNSERVED = [("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32),
            ("vandrs", 10, 1, 8), ("isars", 10, 1, 8), ("vandrs", 17, 4, 8), ("isars", 17, 4, 8),
            ("vandrs", 10, 5, 8), ("isars", 10, 5, 8),
            ("cauchyrs", 10, 1, 8), ("cauchyrs", 30, 3, 8), ("cauchyrs", 10, 4, 32),
            ("liberation", 29, 2, 29)]
FORWARDED = [("vandrs", 10, 4, 8), ("isars", 10, 4, 8), ("vandrs", 4, 2, 8), ("vandrs", 16, 4, 8),
             ("isars", 1, 2, 8)]
BIT_SERVED = [f[:4] for f in W.FAMILIES] + [("cauchyrs", 28, 4, 8), ("cauchyrs", 2, 2, 2)]
# leoec_locate_bitrows: the bitmatrix edge families and the configurations the
# packet condition was worked out on
ROW_CONFIGS = [f[:4] for f in W.FAMILIES] + [
    ("cauchyrs", 4, 2, 8), ("cauchyrs", 4, 2, 3), ("cauchyrs", 10, 4, 5), ("cauchyrs", 5, 3, 5),
    ("cauchyrs", 12, 4, 16), ("cauchyrs", 16, 4, 8), ("cauchyrs", 5, 3, 32),
    ("cauchyrs", 28, 4, 8), ("cauchyrs", 2, 2, 2),
    ("liberation", 2, 2, 3), ("liberation", 3, 2, 3), ("liberation", 4, 2, 5),
    ("liberation", 5, 2, 5), ("liberation", 7, 2, 7), ("liberation", 11, 2, 11),
    ("liberation", 13, 2, 13), ("liberation", 6, 2, 17)]
# worked out on the oracle's bitmatrix as well, but k + m > 2^w: the C ABI
# answers leoec_check_params' status, so the builder is given it directly
ABI_INVALID_ROW_CONFIG = ("cauchyrs", 3, 2, 2)


class Bufs:
    """Host buffers standing in for device memory: no call below gets as far
    as the device, so nothing ever dereferences them."""

    def __init__(self):
        self.store = np.zeros(4096 + 64, dtype=np.uint8)
        self.p = (self.store.ctypes.data + 63) // 64 * 64  # 64-byte aligned


def _locate(le, cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, lost, ws=None,
            ws_bytes=0):
    return le.lib.leoec_locate_ws_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity,
                                      parity_stride, lost, ws, ws_bytes, None)


def _query(le, cid, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    return le.lib.leoec_locate_ws_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out)), out.value


def _rows_rc(le, cid, k, m, w, cap=None):
    cap = (m - 1) * k * w if cap is None else cap
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_locate_bitrows(cid, k, m, w, out, cap), list(out)


def test_helpers_agree_with_the_header(le):
    assert W.MANY == le.device.LOCATE_MANY == 0x80000000
    for cfg in FORWARDED + BIT_SERVED + ROW_CONFIGS:
        assert W.served(*cfg), cfg
    for cfg in UNSERVED:
        assert not W.served(*cfg), cfg
    assert len(W.FAMILIES) == 6 and all(f in H.EDGE_FAMILIES for f in W.FAMILIES)


def test_invalid_parameters_as_check_params(le):
    """Invalid coding or parameters: leoec_check_params' status, ahead of
    every other check (NULL pointers, an empty batch), from all three calls."""
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_check_params(coding, k, m, w)
        assert want < 0
        assert _locate(le, coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, b.p, b.p, 4096) == want
        assert _locate(le, coding, k, m, w, None, 0, 4096, 1, None, 0, None) == want
        assert _locate(le, coding, k, m, w, None, 0, 4096, 0, None, 0, None) == want
        assert _query(le, coding, k, m, w, 4096, 1)[0] == want
        assert le.lib.leoec_locate_ws_dev_workspace(coding, k, m, w, 4096, 1, None) == want
        assert _rows_rc(le, coding, k, m, w, 64)[0] == want
        assert le.lib.leoec_locate_bitrows(coding, k, m, w, None, 0) == want


@pytest.mark.parametrize("cfg", UNSERVED, ids=str)
def test_unserved_configurations(le, cfg):
    """LEOEC_E_UNSUPPORTED without a device, ahead of the pointer checks and
    of the empty batch, from all three calls."""
    cls, k, m, w = cfg
    cid = CID[cls]
    assert le.lib.leoec_check_params(cid, k, m, w) == OK
    b = Bufs()
    bs, _ = le.layout(cls, (k, m, w), 4000)
    assert _locate(le, cid, k, m, w, b.p, 4096, 4000, 1, b.p, m * bs, b.p, b.p, m * bs) == E_UNSUPPORTED
    assert _locate(le, cid, k, m, w, None, 0, 4000, 1, None, 0, None) == E_UNSUPPORTED
    assert _locate(le, cid, k, m, w, None, 0, 4000, 0, None, 0, None) == E_UNSUPPORTED
    assert _query(le, cid, k, m, w, 4000, 1)[0] == E_UNSUPPORTED
    assert le.lib.leoec_locate_ws_dev_workspace(cid, k, m, w, 4000, 1, None) == E_UNSUPPORTED
    assert _rows_rc(le, cid, k, m, w, 1024)[0] == E_UNSUPPORTED
    assert le.lib.leoec_locate_bitrows(cid, k, m, w, None, 0) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.locate_bitrows(cls, (k, m, w))
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.locate_ws_workspace(cls, (k, m, w), 4000, 1)
    assert e.value.code == E_UNSUPPORTED


def test_bitrows_refuses_the_fused_family(le):
    """vandrs / isars have leoec_locate_rows' table, not this one."""
    for cls, k, m, w in FORWARDED:
        assert _rows_rc(le, CID[cls], k, m, w, 1024)[0] == E_UNSUPPORTED
        assert le.lib.leoec_locate_bitrows(CID[cls], k, m, w, None, 0) == E_UNSUPPORTED


def test_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in FORWARDED + BIT_SERVED:
        assert _locate(le, CID[cls], k, m, w, None, 0, 4096, 0, None, 0, None) == OK
        # an empty object has no blocks either
        assert _locate(le, CID[cls], k, m, w, None, 0, 0, 3, None, 0, None) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("isars", 10, 4, 8), ("vandrs", 4, 2, 8),
                                 ("cauchyrs", 10, 4, 8), ("cauchyrs", 6, 3, 4),
                                 ("liberation", 4, 2, 7)], ids=str)
def test_argument_errors(le, cfg):
    """leoec_locate_dev's argument errors with a good workspace; then, for the
    bitmatrix classes, the workspace's own (verify's rules)."""
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    p, ostr, pstr = b.p, 4096, m * bs
    for nobj in (1, 3):
        def call(objs=p, ostr=ostr, par=p, pstr=pstr, lost=p, ws=p, wsb=m * bs):
            return _locate(le, cid, k, m, w, objs, ostr, size, nobj, par, pstr, lost, ws, wsb)
        assert call(objs=None) == E_ARG
        assert call(par=None) == E_ARG
        assert call(lost=None) == E_ARG
        # strides shorter than a row
        assert call(ostr=size - 16) == E_ARG
        assert call(pstr=pstr - 16) == E_ARG
        # misaligned buffers, words and strides
        assert call(objs=p + 8) == E_ARG
        assert call(par=p + 8) == E_ARG
        assert call(lost=p + 2) == E_ARG
        assert call(ostr=ostr + 8) == E_ARG
        assert call(pstr=pstr + 8) == E_ARG
        if cls in ("cauchyrs", "liberation"):
            assert call(ws=None) == E_ARG
            assert call(ws=None, wsb=0) == E_ARG
            assert call(ws=p + 8) == E_ARG
            assert call(wsb=m * bs - 1) == E_ARG
            # the batch's own errors come first
            assert call(objs=None, ws=None) == E_ARG


def test_workspace_query(le):
    size = 1048576 + 77
    for nobj in (0, 1, 5, 2048):
        assert _query(le, CID["vandrs"], 10, 4, 8, size, nobj) == (OK, 0)
        for cls, k, m, w in (("cauchyrs", 10, 4, 8), ("liberation", 4, 2, 7)):
            bs, _ = le.layout(cls, (k, m, w), size)
            assert _query(le, CID[cls], k, m, w, size, nobj) == (OK, nobj * m * bs)
            assert le.device.locate_ws_workspace(cls, (k, m, w), size, nobj) == nobj * m * bs
    assert le.device.locate_ws_workspace("isars", (10, 4, 8), size, 7) == 0
    for cls, k, m, w in (("vandrs", 10, 4, 8), ("cauchyrs", 10, 4, 8), ("liberation", 4, 2, 7)):
        assert le.lib.leoec_locate_ws_dev_workspace(CID[cls], k, m, w, size, 5, None) == E_ARG
    # nobj * m * bs past 2^64
    assert _query(le, CID["cauchyrs"], 10, 4, 8, size, 1 << 62)[0] == E_BAD_SIZE


# ---------------------------------------------------------------------------
# leoec_locate_bitrows

@pytest.mark.parametrize("cfg", ROW_CONFIGS, ids=str)
def test_bitrows_are_the_block_ratios(le, oracle, cfg):
    """None of the configurations is refused; T[i][j] B[0][j] == B[i][j] mod 2
    with B the oracle's bitmatrix, T equals the numpy model's
    B[i][j] B[0][j]^-1, no row names a packet at or above w, and the model
    finds both uniqueness conditions to hold."""
    cls, k, m, w = cfg
    assert (m - 1) * k * w <= W.MAX_WORDS
    B = W.oracle_bitmatrix(oracle, cls, k, m, w)
    assert B.shape == (m * w, k * w)
    T = le.device.locate_bitrows(cls, (k, m, w))
    assert len(T) == m - 1 and all(len(r) == k for r in T)
    assert all(len(x) == w for r in T for x in r)
    for i in range(1, m):
        for j in range(k):
            assert all(x >> w == 0 for x in T[i - 1][j]), (cfg, i, j)
            Tm = W.rows_to_matrix(T[i - 1][j], w).astype(np.int64)
            prod = (Tm @ W.block(B, w, 0, j).astype(np.int64)) & 1
            assert np.array_equal(prod, W.block(B, w, i, j)), (cfg, i, j)
    assert T == W.model_rows(B, k, m, w)
    assert W.unique(B, k, m, w), cfg


def test_bitrows_arguments(le):
    for cls, k, m, w in BIT_SERVED:
        need = (m - 1) * k * w
        assert _rows_rc(le, CID[cls], k, m, w, need)[0] == OK
        assert _rows_rc(le, CID[cls], k, m, w, need - 1)[0] == E_ARG
        assert le.lib.leoec_locate_bitrows(CID[cls], k, m, w, None, need) == E_ARG
        # a larger buffer is filled up to (m-1) k w words and no further; an
        # invertible T has no zero row
        rc, out = _rows_rc(le, CID[cls], k, m, w, need + 3)
        assert rc == OK and out[need:] == [0, 0, 0] and all(out[:need])


def test_builder_refuses_what_it_cannot_name(le, oracle, tmp_path):
    """locate_build_bitrows itself (plain C++, built here without HIP): a
    bitmatrix with one singular block, or with two equal data columns (a
    singular minor), is LEOEC_E_UNSUPPORTED, as is m = 1; the cauchyrs(10,4,8)
    bitmatrix unchanged gives leoec_locate_bitrows' words, and the oracle's
    cauchyrs(3,2,2) bitmatrix, whose parameters the C ABI refuses, the numpy
    model's."""
    so = str(tmp_path / "liblocate_bitrows_test.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall",
                    os.path.join(HERE, "locate_bitrows_test.cpp"),
                    os.path.join(CSRC, "locate_bitrows.cpp"), os.path.join(CSRC, "codes.cpp"),
                    "-o", so], check=True)
    lib = ctypes.CDLL(so)

    def build(B, k, m, w):
        flat = np.ascontiguousarray(B, dtype=np.uint8)
        assert flat.shape == (m * w, k * w)
        out = (ctypes.c_uint32 * max((m - 1) * k * w, 1))()
        return lib.locate_bitrows_of(flat.ctypes.data_as(ctypes.c_void_p), k, m, w, out), list(out)

    k, m, w = 10, 4, 8
    B = W.oracle_bitmatrix(oracle, "cauchyrs", k, m, w)
    rc, T = build(B, k, m, w)
    flat = [x for rows in le.device.locate_bitrows("cauchyrs", (k, m, w)) for blk in rows
            for x in blk]
    assert rc == OK and T == flat
    # one singular block: row 0 of block (2, 7) made equal to its row 1
    sing = B.copy()
    sing[2 * w, 7 * w:8 * w] = sing[2 * w + 1, 7 * w:8 * w]
    assert W.gf2_rank(W.block(sing, w, 2, 7)) == w - 1
    assert build(sing, k, m, w)[0] == E_UNSUPPORTED
    # two equal data columns: every block stays invertible, the minors of
    # columns 4 and 9 are singular
    twin = B.copy()
    twin[:, 9 * w:10 * w] = twin[:, 4 * w:5 * w]
    assert all(W.gf2_rank(W.block(twin, w, i, 9)) == w for i in range(m))
    assert build(twin, k, m, w)[0] == E_UNSUPPORTED
    # one coding block
    assert build(B[:w], k, 1, w)[0] == E_UNSUPPORTED
    cls, k, m, w = ABI_INVALID_ROW_CONFIG
    assert le.lib.leoec_check_params(CID[cls], k, m, w) < 0
    B = W.oracle_bitmatrix(oracle, cls, k, m, w)
    assert W.unique(B, k, m, w)
    rc, T = build(B, k, m, w)
    assert rc == OK and T == [x for rows in W.model_rows(B, k, m, w) for blk in rows for x in blk]
    # the smallest shapes, by hand: identity blocks in row 0, T = the row-1 blocks
    eye, sw = np.eye(2, dtype=np.uint8), np.array([[0, 1], [1, 1]], dtype=np.uint8)
    small = np.block([[eye, eye], [eye, sw]])
    assert build(small, 2, 2, 2) == (OK, [1, 2, 2, 3])
    assert build(np.block([[eye, eye], [sw, sw]]), 2, 2, 2)[0] == E_UNSUPPORTED


# ---------------------------------------------------------------------------
# The host model

@pytest.fixture(scope="module", params=W.FAMILIES, ids=W.family_id)
def family(request):
    return request.param


def test_model_names_a_damaged_data_block(le, oracle, family):
    """Three bytes of one data block damaged: the model names it and only it;
    one byte of a coding block: that block."""
    cls, k, m, w, B = family
    case = H.edge_case(le, oracle, family[:4], H.edge_sizes(k, w, B)[0], n=1)
    assert W.model_words(oracle, le, case, []) == [0]
    j = min(2, k - 1)
    dmg = [("objs", 0, j * case.bs + c, x) for c, x in ((0, 0x01), (case.bs // 2, 0x80),
                                                        (case.bs - 1, 0x5A))]
    assert W.model_words(oracle, le, case, dmg) == [1 << j]
    for i in range(m):
        dmg = [("parity", 0, i * case.bs + 7, W.BIT)]
        assert W.model_words(oracle, le, case, dmg) == [1 << (k + i)]


def test_model_gives_the_device_tests_words(le, oracle, family):
    """No GPU: for every case of test_device_locate_ws.py the model gives the
    words locate_helpers.expected_calls predicts, unchanged, m = 2 families
    included (their double damage lies in different columns: MANY)."""
    cls, k, m, w, B = family
    calls = 0
    for size in H.edge_sizes(k, w, B):
        case = H.edge_case(le, oracle, family[:4], size)
        for dmg, want in L.expected_calls(case):
            assert len({(wh, o, p) for wh, o, p, _ in dmg}) == len(dmg)
            assert W.model_words(oracle, le, case, dmg) == want, (case.ident(), want)
            calls += 1
    assert calls == 3 * len(H.edge_sizes(k, w, B))
