"""leoec_verify_dev / leoec_verify_dev_workspace: the host logic that runs
before the device is opened (no GPU needed).  The workspace query needs no
device at all; leoec_verify_dev checks layout and parameters first, returns
LEOEC_OK for an empty batch, then refuses bad pointers, strides and
workspaces (LEOEC_E_ARG), and only then opens the device, so every status
below is the same on a machine without one."""
import ctypes

import numpy as np
import pytest

OK, E_ARG = 0, -18
CID = {"cauchyrs": 1, "vandrs": 2, "liberation": 3, "isars": 4}
SIZES = (1, 4097, 1048576, 10 * 8704 - 17)
NOBJ = (1, 5, 2048)


def _query(le, cls, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    rc = le.lib.leoec_verify_dev_workspace(CID[cls], k, m, w, size, nobj, ctypes.byref(out))
    return rc, out.value


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("isars", 10, 4, 8)], ids=str)
def test_workspace_query_fused(le, cfg):
    for size in SIZES:
        for nobj in NOBJ:
            assert _query(le, *cfg, size, nobj) == (OK, 0), (size, nobj)
            assert le.device.verify_workspace(cfg[0], cfg[1:], size, nobj) == 0


@pytest.mark.parametrize("cfg", [("cauchyrs", 10, 4, 8), ("vandrs", 20, 4, 8), ("vandrs", 6, 5, 8),
                                 ("vandrs", 4, 2, 16), ("liberation", 4, 2, 7)], ids=str)
def test_workspace_query_two_pass(le, cfg):
    cls, k, m, w = cfg
    for size in SIZES:
        bs, _ = le.layout(cls, (k, m, w), size)
        for nobj in NOBJ:
            assert _query(le, *cfg, size, nobj) == (OK, nobj * m * bs), (size, nobj)
            assert le.device.verify_workspace(cls, (k, m, w), size, nobj) == nobj * m * bs


def test_workspace_query_errors(le):
    assert _query(le, "vandrs", 10, 4, 8, 4096, 0) == (OK, 0)
    assert _query(le, "cauchyrs", 10, 4, 8, 4096, 0) == (OK, 0)
    assert le.lib.leoec_verify_dev_workspace(2, 10, 4, 8, 4096, 1, None) == E_ARG
    for coding, k, m, w in INVALID:
        out = ctypes.c_uint64(0)
        rc = le.lib.leoec_verify_dev_workspace(coding, k, m, w, 4096, 1, ctypes.byref(out))
        assert rc == le.lib.leoec_check_params(coding, k, m, w) and rc < 0


# (coding id, k, m, w): one of every parameter status of leoec_check_params
INVALID = [(0, 10, 4, 8), (7, 10, 4, 8), (2, 0, 4, 8), (2, 10, 0, 8), (2, 10, 4, 9),
           (2, 250, 10, 8), (1, 10, 4, 3), (1, 4, 2, 33), (3, 4, 3, 7), (3, 8, 2, 7),
           (3, 4, 2, 9), (3, 4, 2, 37), (4, 10, 4, 16), (4, 250, 10, 8)]


class Bufs:
    """Host buffers standing in for device memory: no call below gets as far
    as the device, so nothing ever dereferences them."""

    def __init__(self):
        self.store = np.zeros(4096 + 64, dtype=np.uint8)
        base = self.store.ctypes.data
        self.p = (base + 63) // 64 * 64  # 64-byte aligned


def _verify(le, cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, flags, ws,
            ws_bytes):
    return le.lib.leoec_verify_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity,
                                   parity_stride, flags, ws, ws_bytes, None)


def test_verify_invalid_parameters_as_encode(le):
    """Invalid coding or parameters: the statuses of leoec_encode_dev, ahead
    of every other check (NULL pointers included)."""
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_encode_dev(coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, None)
        assert want < 0 and want == le.lib.leoec_check_params(coding, k, m, w)
        assert _verify(le, coding, k, m, w, b.p, 4096, 4096, 1, b.p, 4096, b.p, b.p, 4096) == want
        assert _verify(le, coding, k, m, w, None, 0, 4096, 1, None, 0, None, None, 0) == want


def test_verify_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in [("vandrs", 10, 4, 8), ("cauchyrs", 10, 4, 8), ("liberation", 4, 2, 7)]:
        assert _verify(le, CID[cls], k, m, w, None, 0, 4096, 0, None, 0, None, None, 0) == OK
        # an empty object has no blocks either
        assert _verify(le, CID[cls], k, m, w, None, 0, 0, 3, None, 0, None, None, 0) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("cauchyrs", 10, 4, 8)], ids=str)
def test_verify_argument_errors(le, cfg):
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    p, ostr, pstr, wsb = b.p, 4096, m * bs, m * bs
    for nobj in (1, 3):
        assert _verify(le, cid, k, m, w, None, ostr, size, nobj, p, pstr, p, p, wsb) == E_ARG
        assert _verify(le, cid, k, m, w, p, ostr, size, nobj, None, pstr, p, p, wsb) == E_ARG
        assert _verify(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, None, p, wsb) == E_ARG
        assert _verify(le, cid, k, m, w, p, size - 16, size, nobj, p, pstr, p, p, wsb) == E_ARG
        assert _verify(le, cid, k, m, w, p, ostr, size, nobj, p, pstr - 16, p, p, wsb) == E_ARG
        # misaligned buffers and strides, as the other device calls refuse them
        assert _verify(le, cid, k, m, w, p + 8, ostr, size, nobj, p, pstr, p, p, wsb) == E_ARG
        assert _verify(le, cid, k, m, w, p, ostr, size, nobj, p, pstr, p + 2, p, wsb) == E_ARG
        assert _verify(le, cid, k, m, w, p, ostr + 8, size, nobj, p, pstr, p, p, wsb) == E_ARG


@pytest.mark.parametrize("cfg", [("cauchyrs", 10, 4, 8), ("vandrs", 20, 4, 8), ("vandrs", 6, 5, 8),
                                 ("vandrs", 4, 2, 16), ("liberation", 4, 2, 7)], ids=str)
def test_verify_two_pass_needs_a_workspace(le, cfg):
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    p, pstr = b.p, m * bs
    for nobj in (1, 3):
        assert _verify(le, cid, k, m, w, p, 4096, size, nobj, p, pstr, p, None, 0) == E_ARG
        assert _verify(le, cid, k, m, w, p, 4096, size, nobj, p, pstr, p, None, 1 << 30) == E_ARG
        assert _verify(le, cid, k, m, w, p, 4096, size, nobj, p, pstr, p, p, m * bs - 1) == E_ARG
        assert _verify(le, cid, k, m, w, p, 4096, size, nobj, p, pstr, p, p, 0) == E_ARG
        assert _verify(le, cid, k, m, w, p, 4096, size, nobj, p, pstr, p, p + 8, m * bs) == E_ARG
