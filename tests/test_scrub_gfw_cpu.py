"""leoec_scrub_gfw_dev / leoec_scrub_gfw_dev_workspace / leoec_scrub_wrows:
everything that needs no device.

The order of checks is leoec_scrub_ws_dev's: layout and parameters (the
statuses of leoec_check_params), then whether the configuration is served
(LEOEC_E_UNSUPPORTED), LEOEC_OK for an empty batch, the pointers and strides
and the workspace (LEOEC_E_ARG) and only then the device, so every status
below is the same on a machine without one.  For the word classes the
workspace query is 16 + round_up(4 nobj, 16) + nobj m block_size and the call
takes anything down to one object's encode region; what leoec_scrub_ws_dev
serves is forwarded to it.

leoec_scrub_wrows is a record of the table the device gets: it is held against
leoec_heal_rows and against the oracle's blocks.  The per-lane arithmetic of
gfw_heal_list (gfw_heal_tile.hpp's portable core) is compiled for the CPU and
run against the oracle's field as a stand-alone program, once more under
ASan + UBSan.  The by-construction words test_device_scrub_gfw.py expects of
the device are held against locate_gfw_helpers' host model."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import gpu_helpers as H
import locate_gfw_helpers as G
import scrub_dev_helpers as D
import scrub_helpers as S
import test_scrub_ws_cpu as TS
from test_locate_ws_cpu import CID, INVALID
from test_scrub_cpu import Bufs

X = D.SCRUB_GFW

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "leo_erasure_amd", "csrc")
OK, E_BAD_ID, E_BAD_SIZE, E_UNSUPPORTED, E_ARG = 0, -12, -13, -14, -18

# valid parameters the call does not serve: m = 1, k + m = 32 (which
# leoec_locate_gfw_dev serves), k + m > 32, and the bitmatrix configurations
# leoec_scrub_ws_dev refuses
UNSERVED = [("vandrs", 10, 1, 16), ("vandrs", 10, 1, 8), ("isars", 10, 1, 8),
            ("vandrs", 16, 16, 32), ("vandrs", 20, 12, 8), ("vandrs", 28, 4, 8),
            ("vandrs", 30, 3, 8), ("vandrs", 29, 4, 16),
            ("cauchyrs", 10, 1, 8), ("cauchyrs", 28, 4, 8), ("cauchyrs", 30, 3, 8),
            ("cauchyrs", 10, 4, 32), ("liberation", 29, 2, 29)]
# class (c)
WORD_SERVED = [f[:4] for f in G.FAMILIES] + [X.LAST[:4], ("vandrs", 27, 4, 8), ("vandrs", 1, 2, 32),
                                              ("vandrs", 15, 16, 16)]
# class (a)
FORWARDED = TS.FUSED_SERVED + TS.BIT_SERVED
WROWS_CONFIGS = [f[:4] for f in G.FAMILIES] + [X.LAST[:4]]

assert max(k + m for _, k, m, w in WORD_SERVED) == 31  # the limit is met
assert all(cfg in TS.UNSERVED for cfg in UNSERVED if cfg[0] in ("cauchyrs", "liberation"))
assert all(G.word_class(*cfg) and cfg[1] + cfg[2] <= 31 for cfg in WORD_SERVED)


def _scrub(le, cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report, totals, ws, ws_bytes):
    return le.lib.leoec_scrub_gfw_dev(cid, k, m, w, objs, ostr, size, nobj, parity, pstr, report,
                                      totals, ws, ws_bytes, None)


def _query(le, cid, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    return le.lib.leoec_scrub_gfw_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out)), out.value


def _all_null(le, cid, k, m, w, size, nobj):
    return _scrub(le, cid, k, m, w, None, 0, size, nobj, None, 0, None, None, None, 0)


def _wrows(le, cid, k, m, w, block, cap=None, surv=True, coef=True):
    cap = k if cap is None else cap
    sv = (ctypes.c_int * max(k, 1))()
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_scrub_wrows(cid, k, m, w, block, sv if surv else None,
                                    out if coef else None, cap)


def test_exports(le):
    names = ("leoec_scrub_gfw_dev_workspace", "leoec_scrub_gfw_dev", "leoec_scrub_wrows")
    assert set(names) <= set(le._lib.EXPORTS)
    for name in names:
        assert getattr(le.lib, name)


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
        assert le.lib.leoec_scrub_gfw_dev_workspace(coding, k, m, w, 4096, 1, None) == want
        assert _wrows(le, coding, k, m, w, 0, cap=1024) == want
        assert _wrows(le, coding, k, m, w, -1, cap=0, surv=False, coef=False) == want


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
    assert le.lib.leoec_scrub_gfw_dev_workspace(cid, k, m, w, 4000, 1, None) == E_UNSUPPORTED
    assert _wrows(le, cid, k, m, w, 0, cap=1 << 10) == E_UNSUPPORTED
    assert _wrows(le, cid, k, m, w, -1, cap=0, surv=False, coef=False) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.scrub_gfw_workspace(cls, (k, m, w), 4000, 1)
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.scrub_wrows(cls, (k, m, w), 0)
    assert e.value.code == E_UNSUPPORTED


def test_k_plus_m_32_is_locate_gfw_s_but_not_scrub_gfw_s(le):
    for cls, k, m, w in (("vandrs", 16, 16, 32), ("vandrs", 20, 12, 8), ("vandrs", 28, 4, 8)):
        assert G.word_class(cls, k, m, w)
        out = ctypes.c_uint64()
        assert le.lib.leoec_locate_gfw_dev_workspace(CID[cls], k, m, w, 4000, 1, ctypes.byref(out)) == OK
        assert _query(le, CID[cls], k, m, w, 4000, 1)[0] == E_UNSUPPORTED


def test_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in WORD_SERVED + FORWARDED:
        assert _all_null(le, CID[cls], k, m, w, 4096, 0) == OK
        # an empty object has no blocks either
        assert _all_null(le, CID[cls], k, m, w, 0, 3) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32), ("vandrs", 20, 4, 8),
                                 ("isars", 17, 4, 8)], ids=str)
def test_argument_errors(le, cfg):
    """Host memory standing in for device memory: no call gets as far as the
    device.  The documented order: the call's own buffers (report, totals,
    workspace: NULL, misaligned, too small, overlapping), then the batch's
    pointers and strides."""
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
        # a workspace one byte below the minimum, the header and index words
        # alone, and none
        assert call(wb=wb - 1) == E_ARG
        assert call(wb=D.head(nobj)) == E_ARG
        assert call(wb=0) == E_ARG
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
    for cls, k, m, w in WORD_SERVED:
        cid = CID[cls]
        bs, _ = le.layout(cls, (k, m, w), size)
        for nobj in (0, 1, 5, 2048):
            want = 16 + (4 * nobj + 15) // 16 * 16 + nobj * m * bs
            assert _query(le, cid, k, m, w, size, nobj) == (OK, want), (cls, k, m, w, nobj)
            assert le.device.scrub_gfw_workspace(cls, (k, m, w), size, nobj) == want
            assert want == D.head(nobj) + le.device.locate_gfw_workspace(cls, (k, m, w), size, nobj)
        assert le.lib.leoec_scrub_gfw_dev_workspace(cid, k, m, w, size, 1, None) == E_ARG
        for nobj in (1 << 62, (1 << 64) - 1, 1 << 50):
            assert _query(le, cid, k, m, w, size, nobj)[0] == E_BAD_SIZE
        with pytest.raises(le.LeoecError) as e:
            le.device.scrub_gfw_workspace(cls, (k, m, w), size, 1 << 62)
        assert e.value.code == E_BAD_SIZE


def test_class_a_is_forwarded(le):
    """What leoec_scrub_ws_dev serves, and the bitmatrix configurations it
    refuses: the query's value and both calls' statuses are that call's."""
    b = Bufs()
    refused = [cfg for cfg in TS.UNSERVED if cfg[0] in ("cauchyrs", "liberation")]
    assert refused
    for cls, k, m, w in FORWARDED + refused:
        cid = CID[cls]
        for nobj in (0, 1, 5, 1 << 20, 1 << 62, (1 << 64) - 1):
            for size in (1, 4000, 1 << 30):
                assert _query(le, cid, k, m, w, size, nobj) == TS._query(le, cid, k, m, w, size, nobj)
        assert le.lib.leoec_scrub_gfw_dev_workspace(cid, k, m, w, 4000, 1, None) == \
            le.lib.leoec_scrub_ws_dev_workspace(cid, k, m, w, 4000, 1, None)
        bs, _ = le.layout(cls, (k, m, w), 4000)
        for args in ((b.objs, 4096, 4000, 1, b.parity, m * bs, None, b.totals, b.ws, 8192),
                     (b.objs, 4096, 4000, 1, b.parity, m * bs, b.report, b.totals, b.ws, 16),
                     (None, 0, 4000, 1, None, 0, b.report, b.totals, b.ws, 8192),
                     (None, 0, 4000, 0, None, 0, None, None, None, 0)):
            assert _scrub(le, cid, k, m, w, *args) == TS._scrub(le, cid, k, m, w, *args), (cls, k, m, w)
        assert _wrows(le, cid, k, m, w, 0, cap=1024) == E_UNSUPPORTED


# ---------------------------------------------------------------------------
# leoec_scrub_wrows

def _heal_rows(le, cid, k, m, w, mask):
    surv, want = (ctypes.c_int * k)(), (ctypes.c_int * (k + m))()
    nwant, index = ctypes.c_int(), ctypes.c_int()
    coef = (ctypes.c_uint32 * (m * k))()
    assert le.lib.leoec_heal_rows(cid, k, m, w, mask, surv, want, ctypes.byref(nwant), coef, m * k,
                                  ctypes.byref(index)) == OK
    assert nwant.value == 1
    return list(surv), list(coef[:k])


@pytest.mark.parametrize("cfg", WROWS_CONFIGS, ids=str)
def test_wrows_rebuild_the_block(le, oracle, cfg):
    """For every block b: surv is the first k ids without b, surv and coef are
    leoec_heal_rows' for the mask 1 << b, and coef applied to the oracle's
    blocks of one object (products from the oracle) gives the oracle's block
    b."""
    cls, k, m, w = cfg
    dt = G.DTYPE[w]
    data = H.rand_bytes(k * 16 * w * 3 - 7, 0x6F3 + k)
    blocks = [np.frombuffer(x, dtype=np.uint8).view(dt) for x in oracle.encode(cls, k, m, w, data)]
    for b in range(k + m):
        surv, coef = le.device.scrub_wrows(cls, (k, m, w), b)
        assert surv == [i for i in range(k + m) if i != b][:k]
        assert (surv, coef) == _heal_rows(le, CID[cls], k, m, w, 1 << b), (cfg, b)
        assert all(c >> w == 0 for c in coef)
        acc = np.zeros_like(blocks[0])
        for s, c in zip(surv, coef):
            if c:
                acc ^= G.gf_mul_words(oracle, c, blocks[s], w)
        assert np.array_equal(acc, blocks[b]), (cfg, b)


def test_wrows_arguments(le):
    for cls, k, m, w in WROWS_CONFIGS:
        cid = CID[cls]
        assert _wrows(le, cid, k, m, w, 0) == OK
        assert _wrows(le, cid, k, m, w, k + m - 1) == OK
        assert _wrows(le, cid, k, m, w, 0, cap=k - 1) == E_ARG
        assert _wrows(le, cid, k, m, w, 0, coef=False) == E_ARG
        assert _wrows(le, cid, k, m, w, 0, surv=False) == E_ARG
        assert _wrows(le, cid, k, m, w, -1) == E_BAD_ID
        assert _wrows(le, cid, k, m, w, k + m) == E_BAD_ID
        # the id is looked at before the buffers
        assert _wrows(le, cid, k, m, w, k + m, cap=0, surv=False, coef=False) == E_BAD_ID
        # a larger buffer is filled up to k words and no further
        sv, out = (ctypes.c_int * k)(), (ctypes.c_uint32 * (k + 3))()
        assert le.lib.leoec_scrub_wrows(cid, k, m, w, 1, sv, out, k + 3) == OK
        assert list(out[k:]) == [0, 0, 0]


# ---------------------------------------------------------------------------
# The kernel's per-lane arithmetic on the CPU.

def _record(oracle, w, coefs, rng):
    """One record of tests/gfw_heal_core_test.cpp's input: len(coefs) inputs
    (c, 16 registers of random words, the zero and the all-ones word among
    them) and the XOR of the oracle's products."""
    top = (1 << w) - 1
    dt = G.DTYPE[w]
    out = struct.pack("<II", w, len(coefs))
    acc = np.zeros(64 * 8 // w, dtype=dt)
    for c in coefs:
        words = rng.integers(0, 1 << w, len(acc), dtype=np.uint64).astype(dt)
        words[int(rng.integers(0, len(words)))] = 0
        words[int(rng.integers(0, len(words)))] = top
        acc ^= G.gf_mul_words(oracle, c, words, w)
        out += struct.pack("<I", c) + words.tobytes()
    return out + acc.tobytes()


def _vectors(oracle, corrupt=False):
    """k = 1, 2 and 30 inputs at every width; zero, one, a top-bit-set and the
    all-ones coefficient among them."""
    rng = np.random.default_rng(2041)
    recs = []
    for w in (8, 16, 32):
        top = (1 << w) - 1
        special = [0, 1, 1 << (w - 1), top, 2, 3, top - 1]
        recs += [_record(oracle, w, [c], rng) for c in special]
        recs += [_record(oracle, w, [c, d], rng) for c, d in ((0, 1), (1, 1), (1 << (w - 1), top),
                                                              (special[5], special[6]))]
        rand = [int(x) for x in rng.integers(1, 1 << w, 30 - len(special), dtype=np.uint64)]
        recs.append(_record(oracle, w, special + rand, rng))
        recs.append(_record(oracle, w, [int(x) for x in rng.integers(1, 1 << w, 30, dtype=np.uint64)], rng))
    if corrupt:
        last = bytearray(recs[-1])
        last[-5] ^= 0x10
        recs[-1] = bytes(last)
    return struct.pack("<I", len(recs)) + b"".join(recs), len(recs) // 3


def _probe_sanitizers(tmp_path):
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o",
                            str(tmp_path / "probe")], input="int main() { return 0; }\n",
                           capture_output=True, text=True, timeout=300)
    return probe.returncode == 0, probe.stderr[-300:]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_core_against_the_oracle(oracle, tmp_path, sanitize):
    """tests/gfw_heal_core_test.cpp, a stand-alone program: gfwheal::mac_in and
    from_domain for W = 8 / 16 / 32 over 1, 2 and 30 inputs must give the XOR
    of the oracle's products; once more built with -fsanitize=address,undefined
    (the program itself: no Python, nothing preloaded)."""
    flags = ["-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas"]
    env = dict(os.environ)
    if sanitize:
        ok, why = _probe_sanitizers(tmp_path)
        if not ok:
            pytest.skip("the compiler has no sanitizer runtime: " + why)
        flags = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas",
                 "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        env.update(ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
                   UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    exe = str(tmp_path / "gfw_heal_core_test")
    r = subprocess.run(["g++"] + flags + [os.path.join(HERE, "gfw_heal_core_test.cpp"),
                                          os.path.join(CSRC, "codes.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    vec = str(tmp_path / "vectors.bin")
    data, per = _vectors(oracle)
    with open(vec, "wb") as f:
        f.write(data)
    run = subprocess.run([exe, vec], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert run.stdout.startswith("ok: %d records of w 8, %d of w 16, %d of w 32" % (per, per, per)), out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]
    # the program does compare: one wrong bit in an expected sum fails it
    with open(vec, "wb") as f:
        f.write(_vectors(oracle, corrupt=True)[0])
    run = subprocess.run([exe, vec], capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 1 and "w 32, 30 inputs" in run.stderr, run.stdout + run.stderr


# ---------------------------------------------------------------------------
# The words the device tests expect, against the host model.

@pytest.fixture(scope="module", params=X.FAMILIES + [X.LAST], ids=G.family_id)
def family(request):
    return request.param


def test_families_have_whole_tiles_and_a_partial_one(family):
    cls, k, m, w, B = family
    assert B == 8704 and B // X.TILE == 2 and B % X.TILE == 512
    assert G.word_class(cls, k, m, w) and k + m <= 31


def test_expected_words_are_the_model_s(le, oracle, family):
    """No GPU: the by-construction words of the position batch, the dense
    batch and the whole-block batch equal locate_gfw_helpers' host model for
    every case test_device_scrub_gfw.py runs."""
    sizes = X.sizes(family)[:1] if family == X.LAST else X.sizes(family)
    for case in X.cases(le, oracle, family, sizes):
        dmg, want, skip = X.position(le, oracle, case)
        assert G.model_words(oracle, le, case, dmg) == want, case.ident()
        dmg, want = D.dense_batch(case)
        assert G.model_words(oracle, le, case, dmg) == want, case.ident()
    for case in X.whole_cases(le, oracle, family, sizes):
        blocks = S.whole_batch(case)
        assert G.words_of(oracle, le, case, S.whole_objects(case, blocks)) == \
            S.whole_words(case, blocks), case.ident()
