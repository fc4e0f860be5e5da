"""leoec_scrub_dev / leoec_scrub_dev_workspace: everything that needs no
device.

The order of checks is leoec_locate_dev's: layout and parameters (the statuses
of leoec_check_params), then whether the configuration is served
(LEOEC_E_UNSUPPORTED), LEOEC_OK for an empty batch, the pointers and strides
(LEOEC_E_ARG) and only then the device, so every status below is the same on a
machine without one.  The workspace query is 16 + round_up(4 nobj, 16)."""
import ctypes

import numpy as np
import pytest

from test_locate_cpu import CID, INVALID

OK, E_BAD_SIZE, E_UNSUPPORTED, E_ARG = 0, -13, -14, -18
# valid parameters the call does not serve (the issue's list): vandrs w = 16 and
# 32, m = 1, k = 17, m = 5, and the bitmatrix classes
UNSERVED = [("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32), ("vandrs", 10, 1, 8), ("isars", 10, 1, 8),
            ("vandrs", 17, 4, 8), ("isars", 17, 4, 8), ("vandrs", 10, 5, 8), ("isars", 10, 5, 8),
            ("cauchyrs", 10, 4, 8), ("liberation", 4, 2, 7)]
SERVED = [("vandrs", 10, 4, 8), ("isars", 10, 4, 8), ("vandrs", 4, 2, 8), ("vandrs", 16, 4, 8),
          ("isars", 1, 2, 8)]


def need(nobj):
    return 16 + (4 * nobj + 15) // 16 * 16


class Bufs:
    """Host memory standing in for device memory: no call below gets as far as
    the device, so nothing ever dereferences it.  Four 64-byte aligned
    regions 8 KiB apart: objs, parity, the words (report, then totals 4 KiB
    further) and the workspace."""

    def __init__(self):
        self.store = np.zeros(4 * 8192 + 64, dtype=np.uint8)
        p = (self.store.ctypes.data + 63) // 64 * 64
        self.objs, self.parity, self.report, self.ws = p, p + 8192, p + 16384, p + 24576
        self.totals = self.report + 4096


def _scrub(le, cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report, totals, ws, ws_bytes):
    return le.lib.leoec_scrub_dev(cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report, totals,
                                  ws, ws_bytes, None)


def _query(le, cid, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    return le.lib.leoec_scrub_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out)), out.value


def _all_null(le, cid, k, m, w, size, nobj):
    return _scrub(le, cid, k, m, w, None, 0, size, nobj, None, 0, None, None, None, 0)


def test_error_codes_are_the_header_s(le):
    assert le.strerror(E_UNSUPPORTED) and le.strerror(E_ARG) and le.strerror(E_BAD_SIZE)
    b = Bufs()
    # the three codes as the existing calls return them
    assert le.lib.leoec_locate_dev(CID["cauchyrs"], 10, 4, 8, None, 0, 4096, 1, None, 0, None,
                                   None) == E_UNSUPPORTED
    assert le.lib.leoec_locate_dev(CID["vandrs"], 10, 4, 8, b.objs, 4096, 4096, 1, b.parity, 4096,
                                   None, None) == E_ARG
    out = ctypes.c_uint64()
    assert le.lib.leoec_locate_ws_dev_workspace(CID["cauchyrs"], 10, 4, 8, 1 << 40, 1 << 40,
                                                ctypes.byref(out)) == E_BAD_SIZE


def test_scrub_invalid_parameters_as_check_params(le):
    """Invalid coding or parameters: leoec_check_params' status, ahead of
    every other check (NULL pointers, an empty batch), from both calls."""
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_check_params(coding, k, m, w)
        assert want < 0
        assert _scrub(le, coding, k, m, w, b.objs, 4096, 4096, 1, b.parity, 4096, b.report, b.totals,
                      b.ws, 4096) == want
        assert _all_null(le, coding, k, m, w, 4096, 1) == want
        assert _all_null(le, coding, k, m, w, 4096, 0) == want
        assert _query(le, coding, k, m, w, 4096, 1)[0] == want
        assert le.lib.leoec_scrub_dev_workspace(coding, k, m, w, 4096, 1, None) == want


@pytest.mark.parametrize("cfg", UNSERVED, ids=str)
def test_scrub_unserved_configurations(le, cfg):
    """LEOEC_E_UNSUPPORTED without a device, ahead of the pointer checks and
    of the empty batch, from both calls and from the Python wrapper."""
    cls, k, m, w = cfg
    cid = CID[cls]
    assert le.lib.leoec_check_params(cid, k, m, w) == OK
    b = Bufs()
    bs, _ = le.layout(cls, (k, m, w), 4000)
    assert _scrub(le, cid, k, m, w, b.objs, 4096, 4000, 1, b.parity, m * bs, b.report, b.totals,
                  b.ws, 4096) == E_UNSUPPORTED
    assert _all_null(le, cid, k, m, w, 4000, 1) == E_UNSUPPORTED
    assert _all_null(le, cid, k, m, w, 4000, 0) == E_UNSUPPORTED
    assert _query(le, cid, k, m, w, 4000, 1)[0] == E_UNSUPPORTED
    assert le.lib.leoec_scrub_dev_workspace(cid, k, m, w, 4000, 1, None) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.scrub_workspace(cls, (k, m, w), 4000, 1)
    assert e.value.code == E_UNSUPPORTED


def test_scrub_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in SERVED:
        assert _all_null(le, CID[cls], k, m, w, 4096, 0) == OK
        # an empty object has no blocks either
        assert _all_null(le, CID[cls], k, m, w, 0, 3) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("isars", 10, 4, 8), ("vandrs", 4, 2, 8)],
                         ids=str)
def test_scrub_argument_errors(le, cfg):
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    o, p, r, t, ws = b.objs, b.parity, b.report, b.totals, b.ws
    ostr, pstr = 4096, m * bs
    for nobj in (1, 3, 5):
        wb = need(nobj)

        def call(objs=o, ostr=ostr, parity=p, pstr=pstr, report=r, totals=t, ws=ws, wb=wb):
            return _scrub(le, cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report, totals, ws, wb)

        # NULL or misaligned report, totals, workspace
        assert call(report=None) == E_ARG
        assert call(totals=None) == E_ARG
        assert call(ws=None) == E_ARG
        assert call(report=r + 2) == E_ARG
        assert call(totals=t + 2) == E_ARG
        assert call(ws=ws + 8) == E_ARG
        assert call(ws=ws + 4) == E_ARG
        # report or totals inside the workspace: at its start, at its last
        # word, and reaching into it from below
        assert call(report=ws) == E_ARG
        assert call(report=ws + 16) == E_ARG
        assert call(report=ws - 4 * nobj + 4) == E_ARG
        assert call(totals=ws) == E_ARG
        assert call(totals=ws + wb - 8) == E_ARG
        assert call(totals=ws - 4) == E_ARG
        assert call(totals=ws + 8192 - 8, wb=8192) == E_ARG
        # inside a workspace said to reach the end of the address space
        assert call(report=ws + 4096, wb=(1 << 64) - 16) == E_ARG
        assert call(totals=ws + 4096, wb=(1 << 64) - 16) == E_ARG
        # a workspace one byte short, and none
        assert call(wb=wb - 1) == E_ARG
        assert call(wb=0) == E_ARG
        # the batch's own pointers and strides, as check_dev_batch gives them
        assert call(objs=None) == E_ARG
        assert call(parity=None) == E_ARG
        assert call(objs=o + 8) == E_ARG
        assert call(parity=p + 8) == E_ARG
        assert call(ostr=ostr + 8) == E_ARG
        assert call(pstr=pstr + 8) == E_ARG
        assert call(ostr=size - 16) == E_ARG
        assert call(pstr=pstr - 16) == E_ARG
    # a block of 2^32 bytes or more: LEOEC_E_BAD_SIZE, after the alignment checks
    huge = k << 32
    hbs, _ = le.layout(cls, (k, m, w), huge)
    assert hbs >= 1 << 32
    assert _scrub(le, cid, k, m, w, o, huge, huge, 1, p, m * hbs, r, t, ws, need(1)) == E_BAD_SIZE
    assert le.lib.leoec_locate_dev(cid, k, m, w, o, huge, huge, 1, p, m * hbs, r, None) == E_BAD_SIZE


def test_scrub_workspace_query(le):
    """16 + round_up(4 nobj, 16); overflow is LEOEC_E_BAD_SIZE; bytes == NULL
    is LEOEC_E_ARG; the size of the objects does not enter."""
    for cls, k, m, w in SERVED:
        cid = CID[cls]
        for nobj, want in ((0, 16), (1, 32), (3, 32), (4, 32), (5, 48), (1 << 20, 16 + (4 << 20))):
            assert need(nobj) == want
            for size in (1, 4000, 1 << 30):
                assert _query(le, cid, k, m, w, size, nobj) == (OK, want), (cls, nobj, size)
            assert le.device.scrub_workspace(cls, (k, m, w), 4000, nobj) == want
        assert le.lib.leoec_scrub_dev_workspace(cid, k, m, w, 4000, 1, None) == E_ARG
        for nobj in (1 << 62, (1 << 62) - 1, (1 << 64) - 1):
            assert _query(le, cid, k, m, w, 4000, nobj)[0] == E_BAD_SIZE
        # the largest count whose bytes fit
        top = ((1 << 64) - 32) // 4
        assert _query(le, cid, k, m, w, 4000, top) == (OK, need(top))
        assert _query(le, cid, k, m, w, 4000, top + 1)[0] == E_BAD_SIZE
        with pytest.raises(le.LeoecError) as e:
            le.device.scrub_workspace(cls, (k, m, w), 4000, 1 << 62)
        assert e.value.code == E_BAD_SIZE


def test_python_wrapper_codes(le):
    """device.scrub_workspace raises LeoecError with the C codes (device.scrub
    itself takes device tensors: test_device_scrub.py)."""
    for coding, k, m, w in INVALID:
        names = [n for n, c in CID.items() if c == coding]
        if not names:
            continue
        with pytest.raises(le.LeoecError) as e:
            le.device.scrub_workspace(names[0], (k, m, w), 4096, 1)
        assert e.value.code == le.lib.leoec_check_params(coding, k, m, w)
    with pytest.raises(le.LeoecError) as e:
        le.device.scrub_workspace("nosuch", (10, 4, 8), 4096, 1)
    assert e.value.code == le._lib.E_INVALID_CODING
    assert set(("leoec_scrub_dev", "leoec_scrub_dev_workspace")) <= set(le._lib.EXPORTS)
