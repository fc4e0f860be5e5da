"""leoec_heal_ws_dev / leoec_heal_ws_dev_workspace / leoec_heal_bitrows /
leoec_heal_wrows: everything that needs no device.

The order of checks is the scrub calls': layout and parameters (the statuses
of leoec_check_params), then whether the configuration is served
(LEOEC_E_UNSUPPORTED: the pattern table above 8 MiB, more than 32 ids),
LEOEC_OK for an empty batch, the pointers and strides, the workspace
(LEOEC_E_ARG, LEOEC_E_BAD_SIZE) and only then the device, so every status
below is the same on a machine without one.

The records of the table the device gets are read through leoec_heal_wrows
(word classes) and leoec_heal_bitrows (packet classes): the former are held
against leoec_heal_rows for every mask of 1..m bits, the latter applied to the
oracle's blocks and held against leoec_scrub_bitrows on one-bit masks.  The
table builder and the rank function are compiled into a stand-alone program
(tests/heal_ws_table_test.cpp), once more under ASan + UBSan."""
import ctypes
import itertools
import os
import subprocess
from math import comb

import numpy as np
import pytest

import gpu_helpers as H
import heal_helpers as HH
import heal_ws_helpers as X
from test_locate_ws_cpu import CID, INVALID
from test_scrub_cpu import Bufs

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "leo_erasure_amd", "csrc")
OK, E_NOT_ENOUGH, E_BAD_ID, E_BAD_SIZE, E_UNSUPPORTED, E_ARG = 0, -9, -12, -13, -14, -18

SERVED = X.SERVED + [f[:4] for f in HH.FAMILIES] + [("vandrs", 10, 1, 16), ("cauchyrs", 10, 1, 8),
                                                    ("vandrs", 30, 2, 8), ("isars", 16, 4, 8),
                                                    ("vandrs", 1, 1, 8), ("liberation", 29, 2, 29),
                                                    ("cauchyrs", 10, 4, 32)]
# valid parameters the call does not serve: a table above 8 MiB, more than 32 ids
UNSERVED = X.REFUSED + [("vandrs", 16, 16, 32), ("vandrs", 20, 12, 8), ("vandrs", 20, 5, 8),
                        ("cauchyrs", 16, 4, 32), ("cauchyrs", 28, 4, 8),
                        ("vandrs", 29, 4, 8), ("vandrs", 20, 13, 16), ("cauchyrs", 28, 5, 8)]


def _heal(le, cid, k, m, w, objs, ostr, size, nobj, parity, pstr, lost, unhealed, totals, ws, wb):
    return le.lib.leoec_heal_ws_dev(cid, k, m, w, objs, ostr, size, nobj, parity, pstr, lost, unhealed,
                                    totals, ws, wb, None)


def _all_null(le, cid, k, m, w, size, nobj):
    return _heal(le, cid, k, m, w, None, 0, size, nobj, None, 0, None, None, None, None, 0)


def _query(le, cid, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    return le.lib.leoec_heal_ws_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out)), out.value


def _bitrows(le, cid, k, m, w, mask, r, cap=None, surv=True, rows=True):
    need = w * ((k * w + 31) // 32)
    cap = need if cap is None else cap
    sv = (ctypes.c_int * max(k, 1))()
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_heal_bitrows(cid, k, m, w, mask, r, sv if surv else None,
                                     out if rows else None, cap)


def _wrows(le, cid, k, m, w, mask, r, cap=None, surv=True, coef=True):
    cap = k if cap is None else cap
    sv = (ctypes.c_int * max(k, 1))()
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_heal_wrows(cid, k, m, w, mask, r, sv if surv else None,
                                   out if coef else None, cap)


def test_exports(le):
    names = ("leoec_heal_ws_dev_workspace", "leoec_heal_ws_dev", "leoec_heal_bitrows",
             "leoec_heal_wrows")
    assert set(names) <= set(le._lib.EXPORTS)
    for name in names:
        assert getattr(le.lib, name)


def test_the_rule_is_the_header_s(le):
    """The lists below agree with the rule a caller evaluates (heal_ws_helpers.
    image_bytes, the header's formula)."""
    for cfg in SERVED:
        assert X.served(*cfg), cfg
    for cfg in UNSERVED:
        assert not X.served(*cfg), cfg
    assert X.image_bytes("vandrs", 20, 4, 8) == 4 * (1104 + 12950 * 88) < 8 << 20
    assert X.image_bytes("vandrs", 20, 5, 8) > 8 << 20


def test_invalid_parameters_as_check_params(le):
    b = Bufs()
    for coding, k, m, w in INVALID:
        want = le.lib.leoec_check_params(coding, k, m, w)
        assert want < 0
        assert _heal(le, coding, k, m, w, b.objs, 4096, 4096, 1, b.parity, 4096, b.report,
                     b.report + 64, b.totals, b.ws, 8192) == want
        assert _all_null(le, coding, k, m, w, 4096, 1) == want
        assert _all_null(le, coding, k, m, w, 4096, 0) == want
        assert _query(le, coding, k, m, w, 4096, 1)[0] == want
        assert le.lib.leoec_heal_ws_dev_workspace(coding, k, m, w, 4096, 1, None) == want
        assert _bitrows(le, coding, k, m, w, 1, 0, cap=1024) == want
        assert _wrows(le, coding, k, m, w, 1, 0, cap=1024) == want


@pytest.mark.parametrize("cfg", UNSERVED, ids=str)
def test_unserved_configurations(le, cfg):
    """LEOEC_E_UNSUPPORTED without a device, ahead of the pointer checks and
    of the empty batch, from the call, the query and the Python wrappers."""
    cls, k, m, w = cfg
    cid = CID[cls]
    assert le.lib.leoec_check_params(cid, k, m, w) == OK
    b = Bufs()
    bs, _ = le.layout(cls, (k, m, w), 4000)
    assert _heal(le, cid, k, m, w, b.objs, 4096, 4000, 1, b.parity, m * bs, b.report, b.report + 64,
                 b.totals, b.ws, 8192) == E_UNSUPPORTED
    assert _all_null(le, cid, k, m, w, 4000, 1) == E_UNSUPPORTED
    assert _all_null(le, cid, k, m, w, 4000, 0) == E_UNSUPPORTED
    assert _query(le, cid, k, m, w, 4000, 1)[0] == E_UNSUPPORTED
    assert le.lib.leoec_heal_ws_dev_workspace(cid, k, m, w, 4000, 1, None) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.heal_ws_workspace(cls, (k, m, w), 4000, 1)
    assert e.value.code == E_UNSUPPORTED
    assert _bitrows(le, cid, k, m, w, 1, 0, cap=1 << 12) == E_UNSUPPORTED
    assert _wrows(le, cid, k, m, w, 1, 0, cap=1 << 12) == E_UNSUPPORTED


def test_served_and_empty_batch_without_device(le):
    for cls, k, m, w in SERVED:
        cid = CID[cls]
        assert _query(le, cid, k, m, w, 4096, 5) == (OK, X.head(5)), (cls, k, m, w)
        assert _all_null(le, cid, k, m, w, 4096, 0) == OK
        # an empty object has no blocks either (leoec_heal_dev's)
        assert _all_null(le, cid, k, m, w, 0, 3) == OK
        # served, not empty: the pointers are looked at
        assert _all_null(le, cid, k, m, w, 4096, 1) == E_ARG


def test_workspace_query(le):
    for cls, k, m, w in SERVED:
        cid = CID[cls]
        for size in (1, 4000, 1048576 + 77):
            for nobj in (0, 1, 3, 4, 5, 2048, 1 << 40):
                want = 16 + (4 * nobj + 15) // 16 * 16
                assert _query(le, cid, k, m, w, size, nobj) == (OK, want)
                assert le.device.heal_ws_workspace(cls, (k, m, w), size, nobj) == want
                if HH.fused(cls, k, m, w) and m >= 2:
                    assert want == le.device.scrub_workspace(cls, (k, m, w), size, nobj)
        assert le.lib.leoec_heal_ws_dev_workspace(cid, k, m, w, 4000, 1, None) == E_ARG
        for nobj in (1 << 62, (1 << 64) - 1, (1 << 62) - 3):
            assert _query(le, cid, k, m, w, 4000, nobj)[0] == E_BAD_SIZE
        with pytest.raises(le.LeoecError) as e:
            le.device.heal_ws_workspace(cls, (k, m, w), 4000, 1 << 62)
        assert e.value.code == E_BAD_SIZE


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 8), ("vandrs", 10, 4, 16), ("cauchyrs", 10, 4, 8),
                                 ("vandrs", 20, 4, 8), ("liberation", 4, 2, 7), ("vandrs", 30, 2, 16)],
                         ids=str)
def test_argument_errors(le, cfg):
    """Host memory standing in for device memory: no call gets as far as the
    device.  The documented order: the words' pointers and the batch's pointers
    and strides, then the workspace."""
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    o, p, ws = b.objs, b.parity, b.ws
    lost, un, t = b.report, b.report + 1024, b.totals
    ostr, pstr = 4096, m * bs
    for nobj in (1, 3, 5):
        wb = X.head(nobj)

        def call(objs=o, ostr=ostr, parity=p, pstr=pstr, lost=lost, un=un, totals=t, ws=ws, wb=wb):
            return _heal(le, cid, k, m, w, objs, ostr, size, nobj, parity, pstr, lost, un, totals, ws, wb)

        assert call(lost=None) == E_ARG
        assert call(un=None) == E_ARG
        assert call(totals=None) == E_ARG
        assert call(un=lost) == E_ARG  # lost == unhealed
        assert call(lost=lost + 2) == E_ARG
        assert call(un=un + 2) == E_ARG
        assert call(totals=t + 2) == E_ARG
        # the batch's own pointers and strides, as check_dev_batch gives them
        assert call(objs=None) == E_ARG
        assert call(parity=None) == E_ARG
        assert call(objs=o + 8) == E_ARG
        assert call(parity=p + 8) == E_ARG
        assert call(ostr=ostr + 8) == E_ARG
        assert call(pstr=pstr + 8) == E_ARG
        assert call(ostr=size - 16) == E_ARG
        assert call(pstr=pstr - 16) == E_ARG
        # the workspace: NULL, misaligned, too small
        assert call(ws=None) == E_ARG
        assert call(ws=ws + 8) == E_ARG
        assert call(ws=ws + 4) == E_ARG
        assert call(wb=wb - 1) == E_ARG
        assert call(wb=16) == E_ARG
        assert call(wb=0) == E_ARG
        # unhealed, totals or lost inside the workspace: at its start, in its
        # index words, at its last word, reaching in from below
        for name in ("un", "lost"):
            assert call(**{name: ws}) == E_ARG
            assert call(**{name: ws + 16}) == E_ARG
            assert call(**{name: ws + wb - 4}) == E_ARG
            assert call(**{name: ws - 4 * nobj + 4}) == E_ARG
            assert call(**{name: ws + 4096, "wb": (1 << 64) - 16}) == E_ARG
        assert call(totals=ws) == E_ARG
        assert call(totals=ws + wb - 8) == E_ARG
        assert call(totals=ws - 4) == E_ARG
        assert call(totals=ws + 4096, wb=(1 << 64) - 16) == E_ARG
    # a block of 2^32 bytes or more: LEOEC_E_BAD_SIZE, after the alignment checks
    huge = k << 32
    hbs, _ = le.layout(cls, (k, m, w), huge)
    assert hbs >= 1 << 32
    assert _heal(le, cid, k, m, w, o, huge, huge, 1, p, m * hbs, lost, un, t, ws, 8192) == E_BAD_SIZE
    # index words that overflow: LEOEC_E_BAD_SIZE, after the workspace's pointer
    assert _heal(le, cid, k, m, w, o, ostr, size, 1 << 62, p, pstr, lost, un, t, ws, 8192) == E_BAD_SIZE
    assert _heal(le, cid, k, m, w, o, ostr, size, 1 << 62, p, pstr, lost, un, t, None, 8192) == E_ARG


# ---------------------------------------------------------------------------
# The records of the word classes against leoec_heal_rows.

def _masks(n, m, must=None):
    for p in range(1, m + 1):
        for c in itertools.combinations(range(n), p):
            if must is None or must in c:
                yield HH.bits(c)


@pytest.mark.parametrize("cfg,must", [(("vandrs", 4, 2, 16), None), (("vandrs", 6, 3, 32), None),
                                      (("vandrs", 6, 5, 8), None), (("vandrs", 30, 2, 16), 31)],
                         ids=str)
def test_word_records_are_heal_rows(le, cfg, must):
    """For every mask of 1..m bits (k + m = 32: those containing id 31) and
    every lost slot: the record's survivors and coefficients are
    leoec_heal_rows' surv and row, its slots the lost ids ascending."""
    cls, k, m, w = cfg
    seen = 0
    for mask in _masks(k + m, m, must):
        surv, want, rows, _ = le.device.heal_rows(cls, (k, m, w), mask)
        assert want == HH.ids_of(mask)
        assert surv == [i for i in range(k + m) if not (mask >> i) & 1][:k]
        for r in range(len(want)):
            assert le.device.heal_wrows(cls, (k, m, w), mask, r) == (surv, rows[r]), (cfg, hex(mask), r)
        seen += 1
    assert seen == (sum(comb(k + m, p) for p in range(1, m + 1)) if must is None else 32)


def test_rows_arguments(le):
    for cls, k, m, w in (("vandrs", 4, 2, 16), ("vandrs", 30, 2, 16), ("cauchyrs", 6, 3, 4),
                         ("cauchyrs", 30, 2, 5), ("liberation", 4, 2, 7)):
        cid = CID[cls]
        f = _bitrows if HH.bitsliced(cls) else _wrows
        other = _wrows if HH.bitsliced(cls) else _bitrows
        n = k + m
        top = HH.bits([n - 1])
        assert f(le, cid, k, m, w, top, 0) == OK
        assert f(le, cid, k, m, w, HH.bits([0, n - 1]), 1) == OK
        assert other(le, cid, k, m, w, top, 0, cap=1 << 12) == E_UNSUPPORTED
        # r outside the mask's bit count
        assert f(le, cid, k, m, w, top, 1) == E_ARG
        assert f(le, cid, k, m, w, top, -1) == E_ARG
        assert f(le, cid, k, m, w, 0, 0) == E_ARG
        # leoec_heal_rows' statuses for a bad mask, ahead of r and the buffers
        assert f(le, cid, k, m, w, HH.bits(range(m + 1)), 0) == E_NOT_ENOUGH
        assert f(le, cid, k, m, w, HH.bits(range(m + 1)), 9, cap=0, surv=False) == E_NOT_ENOUGH
        if n < 32:
            assert f(le, cid, k, m, w, 1 << n, 0) == E_BAD_ID
            assert f(le, cid, k, m, w, (1 << n) | 1, 5, cap=0) == E_BAD_ID
        assert f(le, cid, k, m, w, top, 0, cap=0) == E_ARG
        assert f(le, cid, k, m, w, top, 0, surv=False) == E_ARG
    assert _bitrows(le, CID["cauchyrs"], 6, 3, 4, 1, 0, rows=False) == E_ARG
    assert _wrows(le, CID["vandrs"], 4, 2, 16, 1, 0, coef=False) == E_ARG
    # the fused family's map is leoec_heal_rows
    assert _wrows(le, CID["vandrs"], 10, 4, 8, 1, 0) == E_UNSUPPORTED
    assert _bitrows(le, CID["vandrs"], 10, 4, 8, 1, 0, cap=1 << 12) == E_UNSUPPORTED


# ---------------------------------------------------------------------------
# The records of the packet classes against the oracle.

def _apply_bitrows(rows, surv, blocks, k, w):
    """Packet t of the lost block = XOR of packet c of block surv[i] over the
    set bits i w + c of row t."""
    ps = len(blocks[0]) // w
    out = np.zeros(w * ps, dtype=np.uint8)
    for t in range(w):
        acc = out[t * ps:(t + 1) * ps]
        for i in range(k):
            for c in range(w):
                col = i * w + c
                if (rows[t][col // 32] >> (col % 32)) & 1:
                    acc ^= blocks[surv[i]][c * ps:(c + 1) * ps]
    return out


@pytest.mark.parametrize("cfg,must", [(("cauchyrs", 6, 3, 4), None), (("liberation", 4, 2, 7), None),
                                      (("cauchyrs", 30, 2, 5), None)], ids=str)
def test_packet_records_rebuild_the_oracle_s_blocks(le, oracle, cfg, must):
    """For every mask of 1..m bits and every lost slot: surv is the first k
    intact ids, and the record's rows applied to the oracle's blocks give the
    oracle's lost block.  On one-bit masks surv and rows are
    leoec_scrub_bitrows' where that call serves the code."""
    cls, k, m, w = cfg
    data = H.rand_bytes(k * 16 * w * 2 - 7, 0x4EA1 + k)
    blocks = [np.frombuffer(x, dtype=np.uint8) for x in oracle.encode(cls, k, m, w, data)]
    for mask in _masks(k + m, m):
        want = HH.ids_of(mask)
        for r, b in enumerate(want):
            surv, rows = le.device.heal_bitrows(cls, (k, m, w), mask, r)
            assert surv == [i for i in range(k + m) if not (mask >> i) & 1][:k]
            assert np.array_equal(_apply_bitrows(rows, surv, blocks, k, w), blocks[b]), (cfg, hex(mask), r)
            if len(want) == 1 and k + m <= 31:
                assert (surv, rows) == le.device.scrub_bitrows(cls, (k, m, w), b), (cfg, b)


# ---------------------------------------------------------------------------
# The rank function.

def _rank(n, mask):
    """first[p] + sum C(b_i, i) (heal_table.hpp)."""
    ids = HH.ids_of(mask)
    return sum(comb(n, q) for q in range(1, len(ids))) + sum(comb(b, i + 1) for i, b in enumerate(ids))


@pytest.mark.parametrize("n,m", [(6, 2), (11, 5), (32, 2)])
def test_rank_is_a_bijection(n, m):
    count = sum(comb(n, p) for p in range(1, m + 1))
    ranks = sorted(_rank(n, mask) for mask in _masks(n, m))
    assert ranks == list(range(count))


def _probe_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o",
                            str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True, timeout=300)
    return probe.returncode == 0, probe.stderr[-300:]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_table_builder_stand_alone(tmp_path, sanitize):
    """tests/heal_ws_table_test.cpp, a stand-alone program: the library's rank
    is a bijection and the walk of the image's own header gives it, every
    record of five images holds its mask's survivors, slots and words, the
    served shapes are served and vandrs(16,15,8)'s is refused; once more built
    with -fsanitize=address,undefined (the program itself: no Python, nothing
    preloaded)."""
    flags = ["-std=c++17", "-O2", "-Wall", "-Werror"]
    env = dict(os.environ)
    if sanitize:
        ok, why = _probe_sanitizers(tmp_path)
        if not ok:
            pytest.skip("the compiler has no sanitizer runtime: " + why)
        flags = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall",
                 "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        env.update(ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    exe = str(tmp_path / "heal_ws_table_test")
    srcs = [os.path.join(HERE, "heal_ws_table_test.cpp")] + \
        [os.path.join(CSRC, f) for f in ("heal_ws_table.cpp", "heal_table.cpp", "codes.cpp")]
    r = subprocess.run(["g++"] + flags + srcs + ["-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert run.stdout.startswith("ok: 3 ranks, 7 images, 9 served, 8 refused"), out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
