"""leoec_update_dev without a device: the statuses and their order, the host
arithmetic as a stand-alone program, and the kernels' code object.

The order of checks (include/leoec.h): layout and parameters (the statuses of
leoec_check_params), LEOEC_OK for nobj, length or size 0, LEOEC_E_BAD_SIZE for a
range past `size`, LEOEC_E_ARG for the pointers, strides and a patch that
overlaps objs or parity, and only then the device: every call below fails
before that, with pointers that are plain numbers, so every status is the same
on a machine without a GPU and nothing is ever launched.

The range split, the lane masks, the packet map, the word multiply and the
lanes of both kernels replayed on the host are tests/update_core_test.cpp, a
stand-alone program, run plain and built with ASan + UBSan (the program itself:
no Python, nothing preloaded)."""
import os
import subprocess

import pytest

import test_locate_ws_code_object as CO
import update_helpers as U
from test_heal_ws_cpu import _probe_sanitizers

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(CO.ROOT, "leo_erasure_amd", "csrc")
OK, E_PARAMS, E_PARAMS_W_RS, E_PARAMS_M2, E_BAD_SIZE, E_ARG = 0, -2, -3, -5, -13, -18
OBJS, PARITY, PATCH = 0x10000000, 0x20000000, 0x30000000  # never dereferenced


def _call(le, cls="vandrs", p=(10, 4, 8), objs=OBJS, obj_stride=None, size=100000, nobj=3,
          parity=PARITY, parity_stride=None, patch=PATCH, patch_stride=None, offset=33, length=100):
    k, m, w = p
    cid = le._lib.CODING_IDS.get(cls, 99)
    bs = le.layout(cls, p, size)[0] if le._lib.lib.leoec_check_params(cid, k, m, w) == 0 else 16
    if obj_stride is None:
        obj_stride = (size + 15) // 16 * 16
    if parity_stride is None:
        parity_stride = m * bs
    if patch_stride is None:
        patch_stride = (offset % 16 + length + 15) // 16 * 16
    return le._lib.lib.leoec_update_dev(cid, k, m, w, objs, obj_stride, size, nobj, parity,
                                        parity_stride, patch, patch_stride, offset, length, None)


def test_exported(le):
    assert "leoec_update_dev" in le._lib.EXPORTS
    with open(os.path.join(CO.ROOT, "include", "leoec.h")) as fh:
        assert "int leoec_update_dev(" in fh.read()


def test_parameters_come_first(le):
    bad = dict(objs=0, parity=0, patch=0, offset=2**64 - 1, length=2)
    assert _call(le, cls="nocode", **bad) == -1
    assert _call(le, p=(0, 4, 8), **bad) == E_PARAMS
    assert _call(le, p=(10, 4, 9), **bad) == E_PARAMS_W_RS
    assert _call(le, cls="liberation", p=(4, 3, 7), **bad) == E_PARAMS_M2
    assert _call(le, cls="isars", p=(10, 4, 16), **bad) == -8


@pytest.mark.parametrize("empty", [dict(nobj=0), dict(length=0), dict(size=0, offset=0, length=0),
                                   dict(size=0, offset=5, length=7)])
def test_empty_calls_are_ok_before_anything_else(le, empty):
    # NULL pointers, broken strides and (size 0) a range past the object: still OK
    assert _call(le, objs=0, parity=0, patch=0, obj_stride=8, parity_stride=8, patch_stride=8,
                 **empty) == OK


def test_range_before_pointers(le):
    null = dict(objs=0, parity=0, patch=0, patch_stride=16)
    assert _call(le, offset=99999, length=2, **null) == E_BAD_SIZE
    assert _call(le, offset=100000, length=1, **null) == E_BAD_SIZE
    assert _call(le, offset=2**64 - 1, length=2, **null) == E_BAD_SIZE   # the sum wraps
    assert _call(le, offset=5, length=2**64 - 1, **null) == E_BAD_SIZE
    assert _call(le, offset=99999, length=1, **null) == E_ARG            # in range: now the pointers


@pytest.mark.parametrize("bad", [
    dict(objs=0), dict(parity=0), dict(patch=0),
    dict(objs=OBJS + 8), dict(parity=PARITY + 4), dict(patch=PATCH + 1),
    dict(obj_stride=100000 - 16), dict(obj_stride=100008), dict(parity_stride=16),
    dict(patch_stride=96),                # < lead + length = 101
    dict(patch_stride=120),               # not a multiple of 16
    dict(patch=OBJS + 2 * 100000 + 64),   # inside objs' extent (rows of 100,000 B)
    dict(patch=OBJS - 2 * 112 - 16),      # the patch's last row reaches into objs
    dict(patch=PARITY + 4 * 10000),       # inside parity's extent
    dict(nobj=2**62),                     # an extent that does not fit 64 bits
], ids=lambda d: "-".join(d))
def test_argument_faults(le, bad):
    assert _call(le, **bad) == E_ARG
    # the same call with a range past the object: the range is reported first
    assert _call(le, **dict(bad, offset=100000)) == E_BAD_SIZE


def test_every_encode_configuration_is_accepted(le):
    """No configuration leoec_encode_dev serves is refused by its parameters:
    every family of the GPU tests fails first on its NULL pointers."""
    for cls, k, m, w, B in U.FAMILIES:
        assert _call(le, cls=cls, p=(k, m, w), objs=0) == E_ARG, (cls, k, m, w)
    assert any(k + m > 32 for _, k, m, _, _ in U.FAMILIES)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_core_stand_alone(tmp_path, sanitize):
    """tests/update_core_test.cpp: split_range over every offset and length of
    a 3-block, w = 4, ps = 16 object against the byte map, the lane masks, the
    packet positions, mul_dword against the host field, and both kernels' lanes
    on exact-size buffers; once more with -fsanitize=address,undefined."""
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
    exe = str(tmp_path / "update_core_test")
    srcs = [os.path.join(HERE, "update_core_test.cpp"), os.path.join(CSRC, "codes.cpp")]
    r = subprocess.run(["g++"] + flags + srcs + ["-o", exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    out = run.stdout + run.stderr
    assert run.returncode == 0, out[-4000:]
    assert run.stdout.startswith("ok: 60144 splits, 3528 lanes, 6736 packet ranges, 1200 coefficients"), out
    assert "runtime error" not in out and "AddressSanitizer" not in out, out[-4000:]


BUILT = {"product": os.path.join(CSRC, "_build", "update.o"),
         "measure": os.path.join(CSRC, "_build_measure", "update.o")}
GF = "_ZN5leoec6detail9gf_updateILi%dELi%dEEEvNS0_9GfUpdArgsIXT_EXT0_EEE"
WANT = sorted([GF % (w, r) for w in (8, 16, 32) for r in (1, 2, 3, 4)] +
              ["_ZN5leoec6detail10bit_updateENS0_10BitUpdArgsE"])


@pytest.mark.parametrize("build", sorted(BUILT))
@pytest.mark.skipif(not all(os.path.exists(p) for p in BUILT.values()), reason="objects not built")
@pytest.mark.skipif(not all(CO._tool(t) for t in CO.TOOLS), reason="ROCm LLVM tools absent")
def test_update_kernels(tmp_path, build):
    """gf_update<8|16|32, 1..4> and bit_update exist for gfx950 in both
    libraries, depend on w and the rows of a launch only (no k), spill nothing
    and use no scratch; bit_update keeps its deltas in dynamic LDS and its 64
    bit-rows in the argument segment."""
    found = {name: md for name, md in CO.kernel_notes(BUILT[build], str(tmp_path)) if name.startswith("_Z")}
    assert sorted(found) == WANT, sorted(found)
    for name, md in found.items():
        assert int(md["vgpr_spill_count"]) == 0, (name, md)
        assert int(md.get("sgpr_spill_count", "0")) == 0, (name, md)
        assert int(md.get("private_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md.get("group_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md.get("agpr_count", "0")) == 0, (name, md)
        assert int(md["wavefront_size"]) == 64, (name, md)
        assert int(md["kernarg_segment_size"]) < 1024, (name, md)
        if "bit_update" in name:
            assert int(md["max_flat_workgroup_size"]) == 64, (name, md)
            assert int(md["vgpr_count"]) <= 64, (name, md)
        else:
            assert int(md["max_flat_workgroup_size"]) == 256, (name, md)
            # w = 8 / 16: 4 waves per SIMD and more; w = 32: 3 (168 VGPRs)
            assert int(md["vgpr_count"]) <= (168 if "ILi32E" in name else 128), (name, md)
