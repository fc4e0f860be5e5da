"""leoec_locate_gfw_dev / leoec_locate_gfw_dev_workspace / leoec_locate_wrows:
everything that needs no device.

leoec_locate_gfw_dev checks layout and parameters first (the statuses of
leoec_check_params), then whether it serves the configuration
(LEOEC_E_UNSUPPORTED), returns LEOEC_OK for an empty batch, refuses bad
pointers, strides and workspaces (LEOEC_E_ARG) and only then opens the device,
so every status below is the same on a machine without one.  What
leoec_locate_ws_dev serves is forwarded to it.

leoec_locate_wrows gives the ratios T[i][j] = C[i][j] / C[0][j] in GF(2^w).
The host model of locate_gfw_helpers applies them to the syndromes of
oracle-encoded blocks, word by word, and must give the words
test_device_locate_gfw.py expects of the device
(locate_helpers.expected_calls, unchanged).  The per-lane arithmetic of the
kernel (locate_gfw_impl.hpp's portable core) is compiled for the CPU and run
against the oracle's field as a stand-alone program."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import gpu_helpers as H
import locate_gfw_helpers as G
import locate_helpers as L
import test_locate_ws_cpu as TW

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "leo_erasure_amd", "csrc")
OK, E_BAD_SIZE, E_UNSUPPORTED, E_ARG = 0, -13, -14, -18
CID = TW.CID
INVALID = TW.INVALID

# valid parameters leoec_locate_gfw_dev does not serve: m = 1, k + m > 32, and
# the bitmatrix configurations leoec_locate_ws_dev refuses
UNSERVED = [("vandrs", 10, 1, 16), ("vandrs", 10, 1, 8), ("vandrs", 30, 3, 8), ("vandrs", 29, 4, 16),
            ("cauchyrs", 10, 4, 32), ("liberation", 29, 2, 29)]
# class (c)
WORD_SERVED = [f[:4] for f in G.FAMILIES] + [("vandrs", 16, 15, 8), ("vandrs", 28, 4, 8),
                                              ("vandrs", 1, 2, 32), ("vandrs", 16, 16, 32)]


class Bufs(TW.Bufs):
    pass


def _locate(le, cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, lost, ws=None,
            ws_bytes=0):
    return le.lib.leoec_locate_gfw_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity,
                                       parity_stride, lost, ws, ws_bytes, None)


def _query(le, cid, k, m, w, size, nobj):
    out = ctypes.c_uint64(0xDEAD)
    return le.lib.leoec_locate_gfw_dev_workspace(cid, k, m, w, size, nobj, ctypes.byref(out)), out.value


def _rows_rc(le, cid, k, m, w, cap=None):
    cap = (m - 1) * k if cap is None else cap
    out = (ctypes.c_uint32 * max(cap, 1))()
    return le.lib.leoec_locate_wrows(cid, k, m, w, out, cap), list(out)


def test_exports(le):
    names = ("leoec_locate_gfw_dev_workspace", "leoec_locate_gfw_dev", "leoec_locate_wrows")
    assert set(names) <= set(le._lib.EXPORTS)
    for name in names:
        assert getattr(le.lib, name)


def test_helpers_agree_with_the_header(le):
    for cfg in WORD_SERVED:
        assert G.word_class(*cfg) and G.served(*cfg), cfg
    for cfg in TW.FORWARDED + TW.BIT_SERVED:
        assert G.served(*cfg) and not G.word_class(*cfg), cfg
    for cfg in UNSERVED:
        assert not G.served(*cfg), cfg
    # every family is one of the edge harness' (verify's two-pass shapes) or
    # a new code of a class they cover
    assert len(G.FAMILIES) == 6 and all(G.word_class(*f[:4]) for f in G.FAMILIES)


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
        assert le.lib.leoec_locate_gfw_dev_workspace(coding, k, m, w, 4096, 1, None) == want
        assert _rows_rc(le, coding, k, m, w, 64)[0] == want
        assert le.lib.leoec_locate_wrows(coding, k, m, w, None, 0) == want


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
    assert le.lib.leoec_locate_gfw_dev_workspace(cid, k, m, w, 4000, 1, None) == E_UNSUPPORTED
    assert _rows_rc(le, cid, k, m, w, 1024)[0] == E_UNSUPPORTED
    assert le.lib.leoec_locate_wrows(cid, k, m, w, None, 0) == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.locate_wrows(cls, (k, m, w))
    assert e.value.code == E_UNSUPPORTED
    with pytest.raises(le.LeoecError) as e:
        le.device.locate_gfw_workspace(cls, (k, m, w), 4000, 1)
    assert e.value.code == E_UNSUPPORTED


def test_wrows_refuses_class_a(le):
    """What leoec_locate_ws_dev serves has leoec_locate_rows' or
    leoec_locate_bitrows' table, not this one."""
    for cls, k, m, w in TW.FORWARDED + TW.BIT_SERVED:
        assert _rows_rc(le, CID[cls], k, m, w, 1024)[0] == E_UNSUPPORTED
        assert le.lib.leoec_locate_wrows(CID[cls], k, m, w, None, 0) == E_UNSUPPORTED


def test_empty_batch_is_ok_without_device(le):
    for cls, k, m, w in WORD_SERVED + TW.FORWARDED + TW.BIT_SERVED:
        assert _locate(le, CID[cls], k, m, w, None, 0, 4096, 0, None, 0, None) == OK
        # an empty object has no blocks either
        assert _locate(le, CID[cls], k, m, w, None, 0, 0, 3, None, 0, None) == OK


@pytest.mark.parametrize("cfg", [("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32), ("vandrs", 20, 4, 8),
                                 ("isars", 17, 4, 8), ("vandrs", 10, 4, 8), ("cauchyrs", 6, 3, 4)],
                         ids=str)
def test_argument_errors(le, cfg):
    """The batch's argument errors with a good workspace; then, for the classes
    that need one, the workspace's own, which come after the batch's."""
    cls, k, m, w = cfg
    cid, size = CID[cls], 4000
    bs, _ = le.layout(cls, (k, m, w), size)
    b = Bufs()
    assert m * bs <= 4096
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
        if not L.served(cls, k, m, w):
            assert call(ws=None) == E_ARG
            assert call(ws=None, wsb=0) == E_ARG
            assert call(ws=p + 8) == E_ARG
            assert call(wsb=m * bs - 1) == E_ARG
            # the batch's own errors come first
            assert call(objs=None, ws=None) == E_ARG


def test_workspace_query(le):
    size = 1048576 + 77
    for nobj in (0, 1, 5, 2048):
        for cls, k, m, w in WORD_SERVED:
            bs, _ = le.layout(cls, (k, m, w), size)
            assert _query(le, CID[cls], k, m, w, size, nobj) == (OK, nobj * m * bs)
            assert le.device.locate_gfw_workspace(cls, (k, m, w), size, nobj) == nobj * m * bs
    for cls, k, m, w in WORD_SERVED:
        assert le.lib.leoec_locate_gfw_dev_workspace(CID[cls], k, m, w, size, 5, None) == E_ARG
    # nobj * m * bs past 2^64
    assert _query(le, CID["vandrs"], 10, 4, 16, size, 1 << 62)[0] == E_BAD_SIZE
    assert _query(le, CID["vandrs"], 20, 4, 8, size, 1 << 62)[0] == E_BAD_SIZE


def test_query_is_forwarded(le):
    """Class (a): the value and the statuses of leoec_locate_ws_dev_workspace."""
    size = 1048576 + 77
    for cls, k, m, w in TW.FORWARDED + TW.BIT_SERVED:
        for nobj in (0, 5, 1 << 62):
            assert _query(le, CID[cls], k, m, w, size, nobj) == TW._query(le, CID[cls], k, m, w, size, nobj)
        assert le.lib.leoec_locate_gfw_dev_workspace(CID[cls], k, m, w, size, 5, None) == E_ARG
        assert le.device.locate_gfw_workspace(cls, (k, m, w), size, 5) == \
            le.device.locate_ws_workspace(cls, (k, m, w), size, 5)


# ---------------------------------------------------------------------------
# leoec_locate_wrows

def _matrix(le, cid, k, m, w):
    out, n = (ctypes.c_uint32 * (m * k))(), ctypes.c_int()
    assert le.lib.leoec_coding_matrix(cid, k, m, w, out, m * k, ctypes.byref(n)) == OK
    assert n.value == m * k
    return [list(out[i * k:(i + 1) * k]) for i in range(m)]


def _check_ratio(le, oracle, cls, k, m, w):
    assert G.word_class(cls, k, m, w), (cls, k, m, w)
    C = _matrix(le, CID[cls], k, m, w)
    T = le.device.locate_wrows(cls, (k, m, w))
    assert len(T) == m - 1 and all(len(r) == k for r in T)
    for i in range(1, m):
        for j in range(k):
            assert C[0][j] != 0 and C[i][j] != 0
            assert T[i - 1][j] == oracle.gf_div(C[i][j], C[0][j], w), (cls, k, m, w, i, j)
            assert oracle.gf_mul(T[i - 1][j], C[0][j], w) == C[i][j]


def test_wrows_are_the_matrix_ratios(le, oracle):
    """T[i][j] == C[i][j] / C[0][j] of leoec_coding_matrix, division and
    product from the oracle; none of these is refused for a zero entry or a
    singular minor."""
    for w in (16, 32):
        for k in range(1, 17):
            for m in range(2, 5):
                _check_ratio(le, oracle, "vandrs", k, m, w)
        _check_ratio(le, oracle, "vandrs", 16, 16, w)
    for cls in ("vandrs", "isars"):
        for k in range(17, 29):
            _check_ratio(le, oracle, cls, k, 4, 8)
        for k in range(1, 17):
            for m in range(5, 9):
                _check_ratio(le, oracle, cls, k, m, 8)


def test_wrows_arguments(le):
    for cls, k, m, w in WORD_SERVED:
        need = (m - 1) * k
        assert _rows_rc(le, CID[cls], k, m, w, need)[0] == OK
        assert _rows_rc(le, CID[cls], k, m, w, need - 1)[0] == E_ARG
        assert le.lib.leoec_locate_wrows(CID[cls], k, m, w, None, need) == E_ARG
        # a larger buffer is filled up to (m-1) k words and no further
        rc, out = _rows_rc(le, CID[cls], k, m, w, need + 3)
        assert rc == OK and out[need:] == [0, 0, 0] and all(out[:need])
        assert all(x >> w == 0 for x in out)


def test_builder_refuses_what_it_cannot_name(le, oracle, tmp_path):
    """locate_build_wrows itself (plain C++, built here without HIP), at each
    of the three widths: a matrix with a zero entry or a singular 2 x 2 minor
    is LEOEC_E_UNSUPPORTED, as is m = 1; a served code's matrix with one entry
    changed either way is refused, unchanged it gives leoec_locate_wrows'
    words."""
    so = str(tmp_path / "liblocate_wrows_test.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall",
                    os.path.join(HERE, "locate_wrows_test.cpp"),
                    os.path.join(CSRC, "locate_wrows.cpp"), os.path.join(CSRC, "codes.cpp"),
                    "-o", so], check=True)
    B = ctypes.CDLL(so)

    def build(C, k, m, w):
        flat = (ctypes.c_uint32 * (m * k))(*[x for row in C for x in row])
        out = (ctypes.c_uint32 * max((m - 1) * k, 1))()
        return B.locate_wrows_of(flat, k, m, w, out), list(out)

    for w, (cls, k, m) in ((8, ("vandrs", 20, 4)), (16, ("vandrs", 10, 4)), (32, ("vandrs", 6, 3))):
        top = (1 << w) - 1
        assert build([[1, 2], [1, 3]], 2, 2, w) == (OK, [1, oracle.gf_div(3, 2, w)])
        assert build([[top, 2], [1, top]], 2, 2, w) == \
            (OK, [oracle.gf_div(1, top, w), oracle.gf_div(top, 2, w)])
        assert build([[1, 0], [1, 3]], 2, 2, w)[0] == E_UNSUPPORTED   # a zero entry
        assert build([[1, 2], [0, 3]], 2, 2, w)[0] == E_UNSUPPORTED
        assert build([[1, 2], [2, 4]], 2, 2, w)[0] == E_UNSUPPORTED   # rows in proportion
        assert build([[1, 2]], 2, 1, w)[0] == E_UNSUPPORTED           # one coding block
        C = _matrix(le, CID[cls], k, m, w)
        rc, T = build(C, k, m, w)
        assert rc == OK and [T[i * k:(i + 1) * k] for i in range(m - 1)] == \
            le.device.locate_wrows(cls, (k, m, w))
        zero = [row[:] for row in C]
        zero[2][k - 3] = 0
        assert build(zero, k, m, w)[0] == E_UNSUPPORTED
        # rows 1, 2 and columns 1, k - 1: make the minor singular by solving for one entry
        sing = [row[:] for row in C]
        sing[2][k - 1] = oracle.gf_div(oracle.gf_mul(C[1][k - 1], C[2][1], w), C[1][1], w)
        assert sing[2][k - 1] not in (0, C[2][k - 1])
        assert build(sing, k, m, w)[0] == E_UNSUPPORTED
    assert build([[1, 2], [1, 3]], 2, 2, 4)[0] == E_UNSUPPORTED  # not a word width of these classes


# ---------------------------------------------------------------------------
# The kernel's per-lane arithmetic on the CPU.

def _records(oracle, w, rng):
    """[(c, 16 registers of words, 16 registers of c * words)]: coefficients
    with only bit 0, only bit w - 1 and all bits set, zero, and random ones;
    random words, the zero word among them."""
    top = (1 << w) - 1
    coefs = [1, 1 << (w - 1), top, 0, 2, 3, top - 1] + \
        [int(x) for x in rng.integers(1, 1 << w, 40, dtype=np.uint64)]
    out = []
    for c in coefs:
        words = rng.integers(0, 1 << w, 16 * 32 // w, dtype=np.uint64)
        words[int(rng.integers(0, len(words)))] = 0
        words[int(rng.integers(0, len(words)))] = top
        prod = np.array([oracle.gf_mul(c, int(x), w) for x in words], dtype=np.uint64)
        dt = G.DTYPE[w]
        out.append(struct.pack("<I", c) + words.astype(dt).tobytes() + prod.astype(dt).tobytes())
    return out


def test_core_against_the_oracle(oracle, tmp_path):
    """tests/gfw_locate_core_test.cpp, a stand-alone program: gfwloc::misfit
    for W = 8 on every one of the 65,536 products, for W = 16 / 32 on the
    records above; a product fits, a product with one bit flipped does not."""
    exe = str(tmp_path / "gfw_locate_core_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    os.path.join(HERE, "gfw_locate_core_test.cpp"), os.path.join(CSRC, "codes.cpp"),
                    "-o", exe], check=True)
    rng = np.random.default_rng(2032)
    r16, r32 = _records(oracle, 16, rng), _records(oracle, 32, rng)
    mul8 = bytes(oracle.gf_mul(c, x, 8) for c in range(256) for x in range(256))
    vec = str(tmp_path / "vectors.bin")
    with open(vec, "wb") as f:
        f.write(struct.pack("<II", len(r16), len(r32)) + mul8 + b"".join(r16) + b"".join(r32))
    run = subprocess.run([exe, vec], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: 65536 products of w 8, %d records of w 16, %d of w 32" %
                                 (len(r16), len(r32))), run.stdout
    # the program does compare: one wrong product in the table fails it
    bad = bytearray(mul8)
    bad[0x53 * 256 + 0xCA] ^= 0x04
    with open(vec, "wb") as f:
        f.write(struct.pack("<II", 0, 0) + bytes(bad))
    run = subprocess.run([exe, vec], capture_output=True, text=True)
    assert run.returncode == 1 and "w 8 c 0x53" in run.stderr, run.stdout + run.stderr


# ---------------------------------------------------------------------------
# The host model

@pytest.fixture(scope="module", params=G.FAMILIES, ids=G.family_id)
def family(request):
    return request.param


def test_model_names_a_damaged_block(le, oracle, family):
    """Three bytes of one data block damaged, the high byte of a word among
    them: the model names it and only it; one byte of a coding block: that
    block."""
    cls, k, m, w, B = family
    case = H.edge_case(le, oracle, family[:4], H.edge_sizes(k, w, B)[0], n=1)
    assert G.model_words(oracle, le, case, []) == [0]
    for j in sorted({0, min(2, k - 1), k - 1}):
        dmg = [("objs", 0, j * case.bs + c, x) for c, x in ((w // 8 - 1, 0x80), (case.bs // 2, 0x01),
                                                            (case.bs - 1, 0x5A))]
        assert G.model_words(oracle, le, case, dmg) == [1 << j]
    for i in range(m):
        dmg = [("parity", 0, i * case.bs + 7, G.BIT)]
        assert G.model_words(oracle, le, case, dmg) == [1 << (k + i)]


def test_model_gives_the_device_tests_words(le, oracle, family):
    """No GPU: for every case of test_device_locate_gfw.py's edge harness the
    model gives the words locate_helpers.expected_calls predicts, unchanged,
    the m = 2 family included (its double damage lies in different columns:
    MANY)."""
    cls, k, m, w, B = family
    calls = 0
    for size in H.edge_sizes(k, w, B):
        case = H.edge_case(le, oracle, family[:4], size)
        for dmg, want in L.expected_calls(case):
            assert len({(wh, o, p) for wh, o, p, _ in dmg}) == len(dmg)
            assert G.model_words(oracle, le, case, dmg) == want, (case.ident(), want)
            calls += 1
    assert calls == 3 * len(H.edge_sizes(k, w, B))
