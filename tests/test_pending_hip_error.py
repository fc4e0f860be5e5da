"""A HIP error pending on the calling thread is not the library's business
(include/leoec.h, Conventions): a call's status reflects that call's own work,
a `*_dev` call whose own HIP calls all succeed leaves the caller's pending
error where it was, and a host call is neither failed by it nor leaves a new
one behind.

HIP keeps one sticky last-error slot per thread: any failing call stores its
code there, hipGetLastError returns and clears it.  A launcher that asks the
slot "did my launch fail?" therefore reports whatever failed last on the
thread — torch's own call, a fallback the engine recovered from — as its own
failure.  Every other test of the suite runs on a thread whose slot is clean;
here every library call is made with hipErrorInvalidDevice planted in it.

Planting: hipSetDevice(-1), which the runtime refuses before anything reaches
a device; it changes nothing and runs nothing on the GPU.  The runtime is the
one libleoec.so itself is bound to, reached through the library's own handle
(no second copy is loaded; test_runtime_handle checks it).  Torch checks the
slot after its own launches, so between planting and the library call no
torch operation runs: the existing helpers (gpu_helpers, verify_helpers,
locate_helpers, locate_ws_helpers, heal_helpers, scrub_dev_helpers) build
their arenas as always, and `planted` below wraps the one C entry point under
test: synchronize, plant, assert the slot holds the code, call, peek, clear.
The helpers then compare every byte against the oracle as in their own tests.

One row per launcher family (the kernel named is the one whose launcher the
row reaches): 3 objects each, a ragged size whose block is the smallest with
two tiles of the byte kernels (4 KiB tiles: the first multiple of 16 w bytes
above 4,096).

What the commit before this contract did, measured once on an MI355X with this
file: DESIGN.md, "Launch status and the thread's HIP error"."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import gpu_helpers as H
import heal_helpers as P
import locate_helpers as L
import locate_ws_helpers as W
import scrub_dev_helpers as D
import scrub_helpers as S
import verify_helpers as V

HIP_SUCCESS = 0
HIP_ERROR_INVALID_DEVICE = 101
N = 3  # objects per batch


class Runtime:
    """hipSetDevice / hipPeekAtLastError / hipGetLastError of the HIP runtime
    libleoec.so is bound to: dlsym on the library's own handle searches its
    dependencies."""

    def __init__(self, le):
        self.handle = ctypes.CDLL(le._lib.library_path())
        self.set_device = self.handle.hipSetDevice
        self.set_device.argtypes = [ctypes.c_int]
        self.peek = self.handle.hipPeekAtLastError
        self.peek.argtypes = []
        self.get = self.handle.hipGetLastError
        self.get.argtypes = []
        for f in (self.set_device, self.peek, self.get):
            f.restype = ctypes.c_int

    def plant(self):
        """hipErrorInvalidDevice in the calling thread's slot; the precondition
        of every test here is that the slot then shows it (an assertion)."""
        rc = self.set_device(-1)
        assert rc == HIP_ERROR_INVALID_DEVICE, f"hipSetDevice(-1) returned {rc}"
        seen = self.peek()
        assert seen == HIP_ERROR_INVALID_DEVICE, \
            f"the slot shows {seen} right after a refused hipSetDevice(-1)"


@pytest.fixture(scope="module")
def hip(le, gpu):
    return Runtime(le)


class _Wrapped:
    """device.py's `lib` with one entry point wrapped (see `planted`)."""

    def __init__(self, real, entry, call):
        self._real, self._entry, self._call = real, entry, call

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        return self._call(fn) if name == self._entry else fn


@contextlib.contextmanager
def planted(gpu, le, hip, entry):
    """Inside the block every call of `entry` through leo_erasure_amd.device is
    made with the error planted.  Yields the list of (status, slot after the
    call) pairs; the slot is cleared before control returns to torch."""
    calls = []

    def wrap(fn):
        def call(*args):
            gpu.cuda.synchronize()  # every buffer allocated and filled: no torch call from here
            try:
                hip.plant()
                rc = fn(*args)
                calls.append((rc, hip.peek()))
            finally:
                hip.get()
            return rc
        return call

    dev = le.device
    real = dev.lib
    dev.lib = _Wrapped(real, entry, wrap)
    try:
        yield calls
    finally:
        dev.lib = real
        hip.get()


def _check_calls(calls, entry):
    """The status is OK and the caller's error is still in place."""
    assert calls, f"{entry} was not called"
    for rc, after in calls:
        assert rc == 0, f"{entry} returned {rc} ({'LEOEC_E_HIP' if rc == -17 else 'status'}) " \
                        f"with hipErrorInvalidDevice pending on the thread"
        assert after == HIP_ERROR_INVALID_DEVICE, \
            f"{entry}: the caller's pending error became {after} across the call"


def _block(w):
    """The first multiple of 16 w above 4,096: two tiles of gf8_apply / gfs_apply."""
    return (4096 // (16 * w) + 1) * 16 * w


def _case(le, oracle, cls, k, m, w):
    B = _block(w)
    size = k * B - 17  # a ragged last block, B - 17 valid bytes
    case = H.edge_case(le, oracle, (cls, k, m, w), size, n=N)
    assert case.bs == B and case.n == N
    return case


def _encode(gpu, le, oracle, hip, case):
    with planted(gpu, le, hip, "leoec_encode_dev") as calls:
        err = H.check_encode(gpu, le, case)
    return calls, err


def _decode(erased):
    def run(gpu, le, oracle, hip, case):
        with planted(gpu, le, hip, "leoec_decode_dev") as calls:
            err = H.check_decode(gpu, le, case, erased)
        return calls, err
    return run


def _repair(lost):
    def run(gpu, le, oracle, hip, case):
        with planted(gpu, le, hip, "leoec_repair_dev") as calls:
            err = H.check_repair(gpu, le, case, lost)
        return calls, err
    return run


def _verify(gpu, le, oracle, hip, case):
    assert V.fused(case.cls, *case.params) == (case.cls != "cauchyrs")
    want = V.expected_flags(oracle, case, False)
    with planted(gpu, le, hip, "leoec_verify_dev") as calls:
        got, err = V.run_verify(gpu, le, case, V.damage(case, False))
    if not err and got != want:
        err = f"verify {case.ident()}: flags {got}, expected {want}"
    return calls, err


def _locate(gpu, le, oracle, hip, case):
    dmg = L.with_bit(V.damage(case, False))
    want = L.model_words(oracle, le, case, dmg)
    assert want == [1 << case.k, 1 << (case.k + case.m - 1), 1 << L.last_block(case)]
    work, par = L.damaged_arenas(gpu, case, dmg)
    with planted(gpu, le, hip, "leoec_locate_dev") as calls:
        _, got, err = L.run_locate(gpu, le, case, work, par)
    if not err and got != want:
        err = f"locate {case.ident()}: words {got}, expected {want}"
    return calls, err


def _locate_ws(gpu, le, oracle, hip, case):
    dmg = L.with_bit(V.damage(case, False))
    want = W.model_words(oracle, le, case, dmg)
    assert want == [1 << case.k, 1 << (case.k + case.m - 1), 1 << L.last_block(case)]
    work, par = L.damaged_arenas(gpu, case, dmg)
    with planted(gpu, le, hip, "leoec_locate_ws_dev") as calls:
        _, got, err = W.run_locate_ws(gpu, le, case, work, par)
    if not err and got != want:
        err = f"locate_ws {case.ident()}: words {got}, expected {want}"
    return calls, err


def _heal(gpu, le, oracle, hip, case):
    """The first call of the code uploads its table and loads its code object;
    the planted call then heals fresh damage."""
    masks = P.edge_masks(case.k, case.m)
    assert all(P.recoverable(x, case.k, case.m) for x in masks[1:7])
    first = P.run_heal(gpu, le, case, masks[1:4])
    assert not first, "\n".join(first)
    with planted(gpu, le, hip, "leoec_heal_dev") as calls:
        errors = P.run_heal(gpu, le, case, masks[4:7])
    return calls, "\n".join(errors)


def _scrub(gpu, le, oracle, hip, case):
    """As _heal: a first call, then the planted one on fresh damage (the
    first: data blocks 0..2; the second: coding blocks 0..2)."""
    dmg, want = D.dense_batch(case)
    work, par = L.damaged_arenas(gpu, case, dmg)
    _, first = D.SCRUB.check_scrub(gpu, le, case, work, par, want)
    assert not first, "\n".join(first)
    k = case.k
    dmg = [e for o in range(N) for e in S._entries(case, o, k + o, S.VALUES[:S.HITS])]
    want = [1 << (k + o) for o in range(N)]
    work, par = L.damaged_arenas(gpu, case, dmg)
    with planted(gpu, le, hip, "leoec_scrub_dev") as calls:
        _, errors = D.SCRUB.check_scrub(gpu, le, case, work, par, want)
    return calls, "\n".join(errors)


# (id, entry point, class, k, m, w, the call)
ROWS = [
    ("encode-vandrs-10-4-8:gf8_apply", "leoec_encode_dev", "vandrs", 10, 4, 8, _encode),
    ("encode-vandrs-17-5-8:accumulating,multi-row", "leoec_encode_dev", "vandrs", 17, 5, 8, _encode),
    ("encode-vandrs-6-3-32:gfs_apply", "leoec_encode_dev", "vandrs", 6, 3, 32, _encode),
    ("encode-cauchyrs-10-4-8:gfbit_apply", "leoec_encode_dev", "cauchyrs", 10, 4, 8, _encode),
    ("encode-cauchyrs-5-3-17:bit_apply", "leoec_encode_dev", "cauchyrs", 5, 3, 17, _encode),
    ("encode-liberation-4-2-7:lib_apply", "leoec_encode_dev", "liberation", 4, 2, 7, _encode),
    ("encode-liberation-10-2-11:libb_apply", "leoec_encode_dev", "liberation", 10, 2, 11, _encode),
    ("decode-liberation-4-2-7-[1]:libb_dec_apply", "leoec_decode_dev", "liberation", 4, 2, 7,
     _decode([1])),
    ("decode-vandrs-10-4-8-[0,9]", "leoec_decode_dev", "vandrs", 10, 4, 8, _decode([0, 9])),
    ("repair-isars-10-4-8-[0,13]", "leoec_repair_dev", "isars", 10, 4, 8, _repair([0, 13])),
    ("verify-fused-vandrs-10-4-8", "leoec_verify_dev", "vandrs", 10, 4, 8, _verify),
    ("verify-two-pass-cauchyrs-10-4-8:verify_compare", "leoec_verify_dev", "cauchyrs", 10, 4, 8,
     _verify),
    ("locate-vandrs-10-4-8", "leoec_locate_dev", "vandrs", 10, 4, 8, _locate),
    ("locate_ws-cauchyrs-6-3-4:bit_locate", "leoec_locate_ws_dev", "cauchyrs", 6, 3, 4, _locate_ws),
    ("heal-one-launch-vandrs-10-4-8", "leoec_heal_dev", "vandrs", 10, 4, 8, _heal),
    ("heal-synchronising-cauchyrs-10-4-8", "leoec_heal_dev", "cauchyrs", 10, 4, 8, _heal),
    ("scrub-vandrs-10-4-8", "leoec_scrub_dev", "vandrs", 10, 4, 8, _scrub),
]


@pytest.mark.gpu
def test_runtime_handle(gpu, le, hip):
    """The three functions come from the one HIP runtime of the process, the
    one libleoec.so's own launches go through: they resolve through the
    library's handle to a libamdhip64 image, and the process maps exactly one
    such image."""
    class DlInfo(ctypes.Structure):
        _fields_ = [("dli_fname", ctypes.c_char_p), ("dli_fbase", ctypes.c_void_p),
                    ("dli_sname", ctypes.c_char_p), ("dli_saddr", ctypes.c_void_p)]

    dladdr = ctypes.CDLL(None).dladdr
    dladdr.argtypes = [ctypes.c_void_p, ctypes.POINTER(DlInfo)]
    images = set()
    for f in (hip.set_device, hip.peek, hip.get):
        info = DlInfo()
        assert dladdr(ctypes.cast(f, ctypes.c_void_p), ctypes.byref(info))
        images.add(info.dli_fname.decode())
    assert len(images) == 1 and "libamdhip64" in next(iter(images)), images
    with open("/proc/self/maps") as f:
        mapped = {line.split()[-1] for line in f if "libamdhip64" in line}
    assert len(mapped) == 1, f"more than one HIP runtime in the process: {sorted(mapped)}"
    # (the image dladdr names is the mapped one: same file, whatever the spelling of its path)
    assert os.path.samefile(next(iter(images)), next(iter(mapped)))
    # planting works, and clearing it: the precondition of every test below
    try:
        hip.plant()
    finally:
        assert hip.get() == HIP_ERROR_INVALID_DEVICE
    assert hip.peek() == HIP_SUCCESS


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_device_call_with_pending_error(gpu, le, oracle, hip, row):
    """The call returns LEOEC_OK, the peek afterwards still shows
    hipErrorInvalidDevice, and every output is bit-exact against the oracle."""
    _, entry, cls, k, m, w, run = row
    case = _case(le, oracle, cls, k, m, w)
    try:
        calls, err = run(gpu, le, oracle, hip, case)
    finally:
        hip.get()
    _check_calls(calls, entry)
    assert not err, err
    assert hip.peek() == HIP_SUCCESS


# ---------------------------------------------------------------------------
# Host-memory calls.  They may hand the launch to the queue's dispatcher
# thread, so only status, bytes and "no new error code" are asserted.

def _host_call(hip, fn):
    """fn() with the error planted on this thread; (status, slot afterwards).
    No torch call between planting and the clear."""
    try:
        hip.plant()
        rc = fn()
        after = hip.peek()
    finally:
        hip.get()
    assert rc == 0, f"returned {rc} with hipErrorInvalidDevice pending on the thread"
    assert after in (HIP_SUCCESS, HIP_ERROR_INVALID_DEVICE), f"a new error code in the slot: {after}"


def _ptrs(c, ids):
    return ((ctypes.c_void_p * len(ids))(*[c["blocks"][b].ctypes.data for b in ids]),
            (ctypes.c_int * len(ids))(*ids))


@pytest.mark.gpu
def test_host_encode_with_pending_error(gpu, le, oracle, hip):
    c = H.capi_case(le, oracle, "vandrs", 10, 4, 8, 1 << 20, seed=71)
    k, m, w = c["p"]
    need = (k + m - c["filled"]) * c["bs"]
    out = np.empty(need, dtype=np.uint8)
    gpu.cuda.synchronize()
    _host_call(hip, lambda: le.lib.leoec_encode(c["cid"], k, m, w, c["data"].ctypes.data, c["size"],
                                                out.ctypes.data, out.size))
    assert out.tobytes() == b"".join(c["ref"][c["filled"]:])


@pytest.mark.gpu
def test_host_decode_with_pending_error(gpu, le, oracle, hip):
    """k separate survivor blocks: data blocks 0 and 9 and two coding blocks lost."""
    c = H.capi_case(le, oracle, "vandrs", 10, 4, 8, (1 << 20) + 77, seed=72)
    k, m, w = c["p"]
    ids = [b for b in range(k + m) if b not in (0, 9, 11, 12)][::-1]
    assert len(ids) == k
    ptrs, idv = _ptrs(c, ids)
    out = np.empty(c["size"], dtype=np.uint8)
    gpu.cuda.synchronize()
    _host_call(hip, lambda: le.lib.leoec_decode(c["cid"], k, m, w, ptrs, idv, len(ids), c["bs"],
                                                c["size"], out.ctypes.data))
    assert np.array_equal(out, c["data"])


@pytest.mark.gpu
def test_host_large_repair_with_pending_error(gpu, le, oracle, hip):
    """Repair of [0, 13] on an object of 16 MiB + 5 B, the smallest whose
    blocks leave the zero-copy cap (the failure on record was this shape at
    64 MiB)."""
    c = H.capi_case(le, oracle, "vandrs", 10, 4, 8, (16 << 20) + 5, seed=73)
    k, m, w = c["p"]
    rep = [0, 13]
    avail = [b for b in range(k + m) if b not in rep]
    ptrs, idv = _ptrs(c, avail)
    repv = (ctypes.c_int * 2)(*rep)
    out = np.empty(2 * c["bs"], dtype=np.uint8)
    gpu.cuda.synchronize()
    _host_call(hip, lambda: le.lib.leoec_repair(c["cid"], k, m, w, ptrs, idv, len(avail), c["bs"],
                                                repv, 2, out.ctypes.data))
    assert out.tobytes() == c["ref"][0] + c["ref"][13]
