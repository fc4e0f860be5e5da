"""leoec_read_dev without a device: the statuses and their order, the host
arithmetic as a stand-alone program, and the kernels' code object.

The order of checks (include/leoec.h): layout and parameters (the statuses of
leoec_check_params); the erased list as leoec_decode_dev checks it (LEOEC_E_ARG,
LEOEC_E_BAD_ID, LEOEC_E_NOT_ENOUGH_BLOCKS); LEOEC_OK for nobj, length or size 0;
LEOEC_E_BAD_SIZE for a range past `size`; LEOEC_E_ARG for the pointers, strides
and an out that overlaps objs or parity; and only then the device.  Every call
below that names an earlier status also breaks every later rule, with pointers
that are plain numbers, so every status is the same on a machine without a GPU
and nothing is ever launched; one fully valid call reaches the device and, on a
machine without one, says so.

The grouping of segments, the survivor clip, the column transpose, the launch
split and the lanes of both kernels replayed on the host are
tests/read_core_test.cpp, a stand-alone program, run plain and built with
ASan + UBSan (the program itself: no Python, nothing preloaded)."""
import ctypes
import os
import subprocess

import pytest

import test_locate_ws_code_object as CO
import update_helpers as U
from test_heal_ws_cpu import _probe_sanitizers

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(CO.ROOT, "leo_erasure_amd", "csrc")
OK, E_PARAMS, E_PARAMS_W_RS, E_PARAMS_M2 = 0, -2, -3, -5
E_NOT_ENOUGH, E_BAD_ID, E_BAD_SIZE, E_NO_DEVICE, E_ARG = -9, -12, -13, -16, -18
OBJS, PARITY, OUT = 0x10000000, 0x20000000, 0x30000000  # never dereferenced
NOLIST = object()
LIBERATION_WIDE = ("liberation", 28, 2, 29, 2176 * 29)


def _call(le, cls="vandrs", p=(10, 4, 8), objs=OBJS, obj_stride=None, size=100000, nobj=3,
          parity=PARITY, parity_stride=None, erased=(3,), nerased=None, out=OUT, out_stride=None,
          offset=33, length=100):
    k, m, w = p
    cid = le._lib.CODING_IDS.get(cls, 99)
    bs = le.layout(cls, p, size)[0] if le._lib.lib.leoec_check_params(cid, k, m, w) == 0 else 16
    if obj_stride is None:
        obj_stride = (size + 15) // 16 * 16
    if parity_stride is None:
        parity_stride = m * bs
    if out_stride is None:
        out_stride = (offset % 16 + length + 15) // 16 * 16
    if erased is NOLIST:
        er = None
    else:
        er = (ctypes.c_int * max(len(erased), 1))(*erased)
        if nerased is None:
            nerased = len(erased)
    return le._lib.lib.leoec_read_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                                      er, nerased, offset, length, out, out_stride, None)


# every later rule broken at once: a list with a bad id and too few intact ids comes
# with the call where it is not itself under test
LATER = dict(objs=0, parity=0, out=0, obj_stride=8, parity_stride=8, out_stride=8, offset=2**64 - 1,
             length=2)


def test_exported(le):
    assert "leoec_read_dev" in le._lib.EXPORTS
    with open(os.path.join(CO.ROOT, "include", "leoec.h")) as fh:
        assert "int leoec_read_dev(" in fh.read()
    assert le._lib.lib.leoec_read_dev is not None  # the library exports it
    assert callable(le.device.read)


def test_parameters_come_first(le):
    bad = dict(LATER, erased=(99, 0, 1, 2, 3), nerased=-1)
    assert _call(le, cls="nocode", **bad) == -1
    assert _call(le, p=(0, 4, 8), **bad) == E_PARAMS
    assert _call(le, p=(10, 4, 9), **bad) == E_PARAMS_W_RS
    assert _call(le, cls="liberation", p=(4, 3, 7), **bad) == E_PARAMS_M2
    assert _call(le, cls="isars", p=(10, 4, 16), **bad) == -8


def test_the_erased_list_comes_second(le):
    """In leoec_decode_dev's order: the count and the pointer, the ids, the
    survivors; each with every later rule broken too (empty batch included:
    the list is judged before LEOEC_OK is given for nobj = 0)."""
    for later in (LATER, dict(LATER, nobj=0), dict(LATER, length=0)):
        assert _call(le, erased=(14, 0, 1, 2, 3, 4), nerased=-1, **later) == E_ARG
        assert _call(le, erased=NOLIST, nerased=2, **later) == E_ARG
        assert _call(le, erased=(0, 1, 2, 3, 14), **later) == E_BAD_ID      # 5 erased as well
        assert _call(le, erased=(0, 1, 2, 3, -1), **later) == E_BAD_ID
        assert _call(le, erased=(0, 1, 2, 3, 13), **later) == E_NOT_ENOUGH  # 9 intact ids
        assert _call(le, erased=(0, 10, 11, 12, 13), **later) == E_NOT_ENOUGH
    # a repeated id is one id; a NULL list with no entries is an empty list
    assert _call(le, erased=(0, 0, 0, 0, 0, 13), **dict(LATER, nobj=0)) == OK
    assert _call(le, erased=NOLIST, nerased=0, **dict(LATER, nobj=0)) == OK


@pytest.mark.parametrize("empty", [dict(nobj=0), dict(length=0), dict(size=0, offset=0, length=0),
                                   dict(size=0, offset=5, length=7)])
def test_empty_calls_are_ok_before_the_range_and_the_pointers(le, empty):
    # NULL pointers, broken strides and (size 0) a range past the object: still OK
    assert _call(le, **dict(dict(LATER, offset=2**64 - 1, length=2), **empty)) == OK


def test_range_before_pointers(le):
    null = dict(objs=0, parity=0, out=0, obj_stride=8, parity_stride=8, out_stride=8)
    assert _call(le, offset=99999, length=2, **null) == E_BAD_SIZE
    assert _call(le, offset=100000, length=1, **null) == E_BAD_SIZE
    assert _call(le, offset=2**64 - 1, length=2, **null) == E_BAD_SIZE   # the sum wraps
    assert _call(le, offset=5, length=2**64 - 1, **null) == E_BAD_SIZE
    assert _call(le, offset=99999, length=1, **null) == E_ARG            # in range: now the pointers


@pytest.mark.parametrize("bad", [
    dict(objs=0), dict(parity=0), dict(out=0),
    dict(objs=OBJS + 8), dict(parity=PARITY + 4), dict(out=OUT + 1),
    dict(obj_stride=100000 - 16), dict(obj_stride=100008), dict(parity_stride=16),
    dict(out_stride=96),                # < lead + length = 101
    dict(out_stride=120),               # not a multiple of 16
    dict(out=OBJS + 2 * 100000 + 64),   # inside objs' extent (rows of 100,000 B)
    dict(out=OBJS - 2 * 112 - 16),      # out's last row reaches into objs
    dict(out=PARITY + 4 * 10000),       # inside parity's extent
    dict(nobj=2**62),                   # an extent that does not fit 64 bits
], ids=lambda d: "-".join(d))
def test_argument_faults(le, bad):
    assert _call(le, **bad) == E_ARG
    # the same call with a range past the object: the range is reported first
    assert _call(le, **dict(bad, offset=100000)) == E_BAD_SIZE
    # and with too few intact ids: the list before the range
    assert _call(le, **dict(bad, offset=100000, erased=(0, 1, 2, 3, 4))) == E_NOT_ENOUGH


def test_batch_checks_before_out(le):
    """check_dev_batch's statuses come before out's: a block of 4 GiB is
    LEOEC_E_BAD_SIZE whatever out is."""
    size = 10 * 2**32
    assert _call(le, size=size, out=0, out_stride=8) == E_BAD_SIZE
    assert _call(le, size=size) == E_BAD_SIZE


def test_a_valid_call_reaches_the_device(le):
    """Every check passed: the next status is the device's.  Without a GPU
    that is LEOEC_E_NO_DEVICE; with one the pointers would be dereferenced, so
    the call is made only where there is none."""
    if le._lib.lib.leoec_device() >= 0:
        pytest.skip("a device is present: the valid call would run on plain numbers")
    assert _call(le) == E_NO_DEVICE
    assert _call(le, erased=()) == E_NO_DEVICE
    assert _call(le, erased=(10, 13)) == E_NO_DEVICE
    assert _call(le, cls="liberation", p=(28, 2, 29), erased=(5, 28), size=28 * 2176 * 29 - 17) == E_NO_DEVICE


def test_every_decode_configuration_is_accepted(le):
    """No configuration leoec_decode_dev serves is refused by its parameters:
    every family of the GPU tests fails first on its NULL pointers."""
    for cls, k, m, w, B in U.FAMILIES + [LIBERATION_WIDE]:
        assert _call(le, cls=cls, p=(k, m, w), objs=0, erased=(0,)) == E_ARG, (cls, k, m, w)
    assert any(k + m > 32 for _, k, m, _, _ in U.FAMILIES)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_core_stand_alone(tmp_path, sanitize):
    """tests/read_core_test.cpp: the grouping, the clip, the launch split, the
    column transpose, and both kernels' lanes on exact-size buffers against a
    brute-force decode; once more with -fsanitize=address,undefined."""
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
    exe = str(tmp_path / "read_core_test")
    srcs = [os.path.join(HERE, "read_core_test.cpp"), os.path.join(CSRC, "codes.cpp")]
    r = subprocess.run(["g++"] + flags + srcs + ["-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert run.stdout.startswith("ok: 160 groupings, 1881 clips and parts, 4484232 word ranges, "
                                 "883944 packet ranges"), out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]


BUILT = {"product": os.path.join(CSRC, "_build", "read.o"),
         "measure": os.path.join(CSRC, "_build_measure", "read.o")}
WANT = sorted(["_ZN5leoec6detail10range_copyENS0_8CopyArgsE", "_ZN5leoec6detail8bit_readENS0_9BitRdArgsE"] +
              ["_ZN5leoec6detail7gf_readILi%dEEEvNS0_8GfRdArgsIXT_EEE" % w for w in (8, 16, 32)])


@pytest.mark.parametrize("build", sorted(BUILT))
@pytest.mark.skipif(not all(os.path.exists(p) for p in BUILT.values()), reason="objects not built")
@pytest.mark.skipif(not all(CO._tool(t) for t in CO.TOOLS), reason="ROCm LLVM tools absent")
def test_read_kernels(tmp_path, build):
    """range_copy, gf_read<8|16|32> and bit_read exist for gfx950 in both
    libraries, depend on w only (no k), spill nothing, use no scratch and no
    static LDS (bit_read's accumulators are dynamic LDS), and keep their
    argument segment within 3,200 bytes."""
    found = {name: md for name, md in CO.kernel_notes(BUILT[build], str(tmp_path)) if name.startswith("_Z")}
    assert sorted(found) == WANT, sorted(found)
    for name, md in found.items():
        assert int(md["vgpr_spill_count"]) == 0, (name, md)
        assert int(md.get("sgpr_spill_count", "0")) == 0, (name, md)
        assert int(md.get("private_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md.get("group_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md["wavefront_size"]) == 64, (name, md)
        assert int(md["kernarg_segment_size"]) <= 3200, (name, md)
        assert int(md["max_flat_workgroup_size"]) == (64 if "bit_read" in name else 256), (name, md)
        assert int(md["vgpr_count"]) <= 128, (name, md)  # 4 waves per SIMD and more
