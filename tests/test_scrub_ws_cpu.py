"""leoec_scrub_ws_dev / leoec_scrub_ws_dev_workspace / leoec_scrub_bitrows:
everything that needs no device.

The order of checks is leoec_scrub_dev's: layout and parameters (the statuses
of leoec_check_params), then whether the configuration is served
(LEOEC_E_UNSUPPORTED), LEOEC_OK for an empty batch, the pointers and strides
(LEOEC_E_ARG) and only then the device, so every status below is the same on a
machine without one.  For cauchyrs and liberation the workspace query is
16 + round_up(4 nobj, 16) + nobj m block_size and the call takes anything down
to one object's encode region.  leoec_scrub_bitrows is held against a numpy
GF(2) model built from the oracle's bitmatrix; bit_heal_list's code object
against the resources its shape promises; the host-only table builder runs
under ASan + UBSan as a program of its own."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import locate_ws_helpers as W
import scrub_dev_helpers as D
from test_locate_ws_code_object import TOOLS, _tool, kernel_notes
from test_locate_ws_cpu import CID, INVALID
from test_locate_ws_cpu import UNSERVED as LOCATE_WS_UNSERVED
from test_scrub_cpu import SERVED as FUSED_SERVED
from test_scrub_cpu import Bufs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "leo_erasure_amd", "csrc")
OK, E_BAD_ID, E_BAD_SIZE, E_UNSUPPORTED, E_ARG = 0, -12, -13, -14, -18
# valid parameters the call does not serve: leoec_locate_ws_dev's list, and
# k + m = 32, which that call serves
UNSERVED = LOCATE_WS_UNSERVED + [("cauchyrs", 28, 4, 8)]
BIT_SERVED = [f[:4] for f in W.FAMILIES] + [("cauchyrs", 2, 2, 2), ("cauchyrs", 27, 4, 8)]


assert ("liberation", 29, 2, 29) in UNSERVED and ("cauchyrs", 10, 4, 32) in UNSERVED
assert max(k + m for _, k, m, w in BIT_SERVED) == 31  # the limit is met


def _scrub(le, cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report, totals, ws, ws_bytes):
    return le.lib.leoec_scrub_ws_dev(cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report,
                                     totals, ws, ws_bytes, None)


def _query(le, cid, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    return le.lib.leoec_scrub_ws_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out)), out.value


def _all_null(le, cid, k, m, w, size, nobj):
    return _scrub(le, cid, k, m, w, None, 0, size, nobj, None, 0, None, None, None, 0)


def _bitrows(le, cid, k, m, w, block, cap=None, surv=True, rows=True):
    rw = (k * w + 31) // 32
    cap = w * rw if cap is None else cap
    sv = (ctypes.c_int * max(k, 1))()
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_scrub_bitrows(cid, k, m, w, block, sv if surv else None,
                                      out if rows else None, cap)


def test_exports(le):
    assert set(("leoec_scrub_ws_dev", "leoec_scrub_ws_dev_workspace", "leoec_scrub_bitrows")) <= \
        set(le._lib.EXPORTS)


def test_invalid_parameters_as_check_params(le):
    """Invalid coding or parameters: leoec_check_params' status, ahead of
    every other check (NULL pointers, an empty batch), from all three calls."""
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_check_params(coding, k, m, w)
        assert want < 0
        assert _scrub(le, coding, k, m, w, b.objs, 4096, 4096, 1, b.parity, 4096, b.report, b.totals,
                      b.ws, 8192) == want
        assert _all_null(le, coding, k, m, w, 4096, 1) == want
        assert _all_null(le, coding, k, m, w, 4096, 0) == want
        assert _query(le, coding, k, m, w, 4096, 1)[0] == want
        assert le.lib.leoec_scrub_ws_dev_workspace(coding, k, m, w, 4096, 1, None) == want
        assert _bitrows(le, coding, k, m, w, 0, cap=1024) == want
        names = [n for n, c in CID.items() if c == coding]
        if names:
            with pytest.raises(le.LeoecError) as e:
                le.device.scrub_ws_workspace(names[0], (k, m, w), 4096, 1)
            assert e.value.code == want


@pytest.mark.parametrize("cfg", UNSERVED, ids=str)
def test_unserved_configurations(le, cfg):
    """LEOEC_E_UNSUPPORTED without a device, ahead of the pointer checks and
    of the empty batch, from all three calls and from the Python wrappers."""
    cls, k, m, w = cfg
    cid = CID[cls]
    assert le.lib.leoec_check_params(cid, k, m, w) == OK
    b = Bufs()
    bs, _ = le.layout(cls, (k, m, w), 4000)
    assert _scrub(le, cid, k, m, w, b.objs, 4096, 4000, 1, b.parity, m * bs, b.report, b.totals,
                  b.ws, 8192) == E_UNSUPPORTED
    assert _all_null(le, cid, k, m, w, 4000, 1) == E_UNSUPPORTED
    assert _all_null(le, cid, k, m, w, 4000, 0) == E_UNSUPPORTED
    assert _query(le, cid, k, m, w, 4000, 1)[0] == E_UNSUPPORTED
    assert le.lib.leoec_scrub_ws_dev_workspace(cid, k, m, w, 4000, 1, None) == E_UNSUPPORTED
    assert _bitrows(le, cid, k, m, w, 0, cap=1 << 16) == E_UNSUPPORTED
    assert _bitrows(le, cid, k, m, w, -1, cap=0, surv=False, rows=False) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.scrub_ws_workspace(cls, (k, m, w), 4000, 1)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.scrub_bitrows(cls, (k, m, w), 0)
    assert e.value.code == E_UNSUPPORTED


def test_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in FUSED_SERVED + BIT_SERVED:
        assert _all_null(le, CID[cls], k, m, w, 4096, 0) == OK
        # an empty object has no blocks either
        assert _all_null(le, CID[cls], k, m, w, 0, 3) == OK


@pytest.mark.parametrize("cfg", [("cauchyrs", 10, 4, 8), ("liberation", 4, 2, 7),
                                 ("cauchyrs", 5, 3, 17)], ids=str)
def test_argument_errors(le, cfg):
    """Host memory standing in for device memory: no call gets as far as the
    device."""
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    o, p, r, t, ws = b.objs, b.parity, b.report, b.totals, b.ws
    ostr, pstr = 4096, m * bs
    for nobj in (1, 3, 5):
        wb = D.head(nobj) + m * bs  # the minimum
        assert wb <= 8192

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
        # report or totals inside the workspace: at its start, in its index
        # words, in its encode region, at its last word, reaching in from below
        assert call(report=ws) == E_ARG
        assert call(report=ws + 16) == E_ARG
        assert call(report=ws + D.head(nobj)) == E_ARG
        assert call(report=ws - 4 * nobj + 4) == E_ARG
        assert call(totals=ws) == E_ARG
        assert call(totals=ws + wb - 8) == E_ARG
        assert call(totals=ws - 4) == E_ARG
        assert call(totals=ws + 8192 - 8, wb=8192) == E_ARG
        # inside a workspace said to reach the end of the address space
        assert call(report=ws + 4096, wb=(1 << 64) - 16) == E_ARG
        assert call(totals=ws + 4096, wb=(1 << 64) - 16) == E_ARG
        # a workspace one byte below the minimum, the header and index words
        # alone, and none
        assert call(wb=wb - 1) == E_ARG
        assert call(wb=D.head(nobj)) == E_ARG
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
    assert _scrub(le, cid, k, m, w, o, huge, huge, 1, p, m * hbs, r, t, ws,
                  D.head(1) + m * hbs) == E_BAD_SIZE


def test_workspace_query(le):
    size = 1048576 + 77
    for cls, k, m, w in BIT_SERVED:
        cid = CID[cls]
        bs, _ = le.layout(cls, (k, m, w), size)
        for nobj in (0, 1, 3, 4, 5, 2048):
            want = 16 + (4 * nobj + 15) // 16 * 16 + nobj * m * bs
            assert _query(le, cid, k, m, w, size, nobj) == (OK, want), (cls, k, m, w, nobj)
            assert le.device.scrub_ws_workspace(cls, (k, m, w), size, nobj) == want
            locate = ctypes.c_uint64()
            assert le.lib.leoec_locate_ws_dev_workspace(cid, k, m, w, size, nobj,
                                                        ctypes.byref(locate)) == OK
            assert want == D.head(nobj) + locate.value
        assert le.lib.leoec_scrub_ws_dev_workspace(cid, k, m, w, size, 1, None) == E_ARG
        for nobj in (1 << 62, (1 << 64) - 1, 1 << 50):
            assert _query(le, cid, k, m, w, size, nobj)[0] == E_BAD_SIZE
        assert _query(le, cid, k, m, w, 1 << 40, 1 << 40)[0] == E_BAD_SIZE
        with pytest.raises(le.LeoecError) as e:
            le.device.scrub_ws_workspace(cls, (k, m, w), size, 1 << 62)
        assert e.value.code == E_BAD_SIZE


def test_workspace_query_forwards_the_fused_family(le):
    """For everything leoec_scrub_dev serves the query is that call's."""
    for cls, k, m, w in FUSED_SERVED:
        cid = CID[cls]
        for nobj in (0, 1, 5, 1 << 20, 1 << 62, (1 << 64) - 1):
            for size in (1, 4000, 1 << 30):
                out = ctypes.c_uint64(0xDEAD)
                rc = le.lib.leoec_scrub_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out))
                assert _query(le, cid, k, m, w, size, nobj) == (rc, out.value)
        assert le.lib.leoec_scrub_ws_dev_workspace(cid, k, m, w, 4000, 1, None) == E_ARG


# ---------------------------------------------------------------------------
# leoec_scrub_bitrows against a numpy GF(2) model.

@pytest.mark.parametrize("cfg", BIT_SERVED, ids=str)
def test_bitrows_rebuild_the_block(le, oracle, cfg):
    """With G = [I; B], B the oracle's bitmatrix: for every block b, surv is
    the first k ids without b and rows x G[surv] == G[b] over GF(2)."""
    cls, k, m, w = cfg
    B = np.array(W.oracle_bitmatrix(oracle, cls, k, m, w), dtype=np.uint8).reshape(m * w, k * w) & 1
    G = np.concatenate([np.eye(k * w, dtype=np.uint8), B], axis=0).astype(np.int64)
    rw = (k * w + 31) // 32
    for b in range(k + m):
        surv, rows = le.device.scrub_bitrows(cls, (k, m, w), b)
        assert surv == [i for i in range(k + m) if i != b][:k]
        assert len(rows) == w and all(len(r) == rw for r in rows)
        R = np.array([[(row[c // 32] >> (c % 32)) & 1 for c in range(rw * 32)] for row in rows],
                     dtype=np.int64)
        assert not R[:, k * w:].any()
        Gs = np.concatenate([G[s * w:(s + 1) * w] for s in surv], axis=0)
        assert np.array_equal((R[:, :k * w] @ Gs) & 1, G[b * w:(b + 1) * w]), (cfg, b)


def test_bitrows_arguments(le):
    for cls, k, m, w in BIT_SERVED:
        cid = CID[cls]
        need = w * ((k * w + 31) // 32)
        assert _bitrows(le, cid, k, m, w, 0) == OK
        assert _bitrows(le, cid, k, m, w, k + m - 1) == OK
        assert _bitrows(le, cid, k, m, w, 0, cap=need - 1) == E_ARG
        assert _bitrows(le, cid, k, m, w, 0, rows=False) == E_ARG
        assert _bitrows(le, cid, k, m, w, 0, surv=False) == E_ARG
        assert _bitrows(le, cid, k, m, w, -1) == E_BAD_ID
        assert _bitrows(le, cid, k, m, w, k + m) == E_BAD_ID
        # the id is looked at before the buffers
        assert _bitrows(le, cid, k, m, w, k + m, cap=0, surv=False, rows=False) == E_BAD_ID


def test_bitrows_refuses_the_fused_family(le):
    """vandrs / isars have leoec_heal_rows' map, not this one."""
    for cls, k, m, w in FUSED_SERVED:
        assert _bitrows(le, CID[cls], k, m, w, 0, cap=1024) == E_UNSUPPORTED
        assert _bitrows(le, CID[cls], k, m, w, 99, cap=0, surv=False, rows=False) == E_UNSUPPORTED


# ---------------------------------------------------------------------------
# The code object.

OBJ = os.path.join(CSRC, "_build", "scrub.o")


@pytest.mark.skipif(not os.path.exists(OBJ), reason="product objects not built")
@pytest.mark.skipif(not all(_tool(t) for t in TOOLS), reason="ROCm LLVM tools absent")
def test_bit_heal_list_code_object(tmp_path):
    """One instance (w, k and m are runtime values); its accumulators are in
    LDS sized at the launch, so no register array is indexed by w: no spill,
    no scratch, no static LDS; the table is in memory, so the argument segment
    is small; one wave per workgroup."""
    notes = kernel_notes(OBJ, str(tmp_path))
    found = [(name, md) for name, md in notes if "bit_heal_list" in name and name.startswith("_Z")
             and "vgpr_spill_count" in md]
    assert len(found) == 1, [name for name, _ in found]
    name, md = found[0]
    assert "bit_locate" not in name
    assert int(md["vgpr_spill_count"]) == 0, md
    assert int(md.get("sgpr_spill_count", "0")) == 0, md
    assert int(md.get("private_segment_fixed_size", "0")) == 0, md
    assert int(md.get("group_segment_fixed_size", "0")) == 0, md
    assert int(md["kernarg_segment_size"]) < 4096, md
    assert int(md["max_flat_workgroup_size"]) == 64, md
    # none of the six families test_built_kernels_are_the_inventory counts
    for fam in ("gfbit_apply", "gfs_apply", "lib_apply", "libb_apply", "libb_dec_apply", "bit_apply"):
        assert not any(fam in n for n, _ in notes), fam


# ---------------------------------------------------------------------------
# The host-only table builder under ASan + UBSan, as a program of its own.

def test_table_builder_under_sanitizers(tmp_path):
    src = [os.path.join(HERE, "host_sanitize", "scrub_bit_table_main.cpp"),
           os.path.join(CSRC, "scrub_bit_table.cpp"), os.path.join(CSRC, "codes.cpp")]
    exe = str(tmp_path / "scrub_bit_table")
    flags = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o",
                            str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True, timeout=300)
    if probe.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + probe.stderr[-300:])
    r = subprocess.run(["g++"] + flags + ["-o", exe] + src, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    args = []
    for cls, k, m, w in BIT_SERVED:
        args += [cls[0], str(k), str(m), str(w)]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-6000:]
    assert "scrub_bit_table: all checks held" in r.stdout, out[-3000:]
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-6000:]
