"""A HIP error pending on the calling thread, for the tests of one device call
(test_device_scrub_ws.py, test_device_scrub_gfw.py, test_device_heal_ws.py):
test_pending_hip_error.py's way, hipSetDevice(-1) through the library's own
runtime handle, no torch call between planting and the clear."""
import contextlib
import ctypes

HIP_SUCCESS, HIP_ERROR_INVALID_DEVICE = 0, 101


class _Wrapped:
    """device.py's `lib` with the entry point `entry` wrapped."""

    def __init__(self, real, entry, call):
        self._real, self._entry, self._call = real, entry, call

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        return self._call(fn) if name == self._entry else fn


@contextlib.contextmanager
def planted(gpu, le, calls, entry):
    """Inside the block every call of `entry` through leo_erasure_amd.device
    is made with hipErrorInvalidDevice planted; `calls` takes (status, slot
    after the call) of each.  Yields the runtime handle; the slot is cleared
    before control returns to torch."""
    rt = ctypes.CDLL(le._lib.library_path())
    for f in (rt.hipSetDevice, rt.hipPeekAtLastError, rt.hipGetLastError):
        f.restype = ctypes.c_int
    rt.hipSetDevice.argtypes = [ctypes.c_int]

    def wrap(fn):
        def call(*args):
            gpu.cuda.synchronize()  # every buffer allocated and filled: no torch call from here
            try:
                assert rt.hipSetDevice(-1) == HIP_ERROR_INVALID_DEVICE
                assert rt.hipPeekAtLastError() == HIP_ERROR_INVALID_DEVICE
                rc = fn(*args)
                calls.append((rc, rt.hipPeekAtLastError()))
            finally:
                rt.hipGetLastError()
            return rc
        return call

    dev = le.device
    real = dev.lib
    dev.lib = _Wrapped(real, entry, wrap)
    try:
        yield rt
    finally:
        dev.lib = real
        rt.hipGetLastError()
