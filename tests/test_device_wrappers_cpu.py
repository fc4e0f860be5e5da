"""leo_erasure_amd/device.py without a device: what each wrapper of the
verify / heal / locate / scrub calls checks, allocates and passes to the
library, in which order, pinned with stand-ins for `device.lib` and
`device.torch`.  The library entries record (name, arguments) and return
LEOEC_OK; a `*_workspace` query answers `lib.need`; the rows entries fill
every array with 0, 1, 2, ...  Arguments are recorded as plain values: a
c_void_p as ("vp", value), a byref as "out", an array as (element type,
length)."""
import ctypes
import types

import pytest

INT32, UINT8 = "int32", "uint8"
STREAM = ("vp", 0x5EED)  # the current stream of the stand-in torch


class Tensor:
    def __init__(self, dtype, n, ptr, contiguous=True, stride=None):
        self.dtype, self.is_cuda, self.device = dtype, True, types.SimpleNamespace(index=0)
        self.shape = n if isinstance(n, tuple) else (n,)
        self._stride = stride or (self.shape[-1], 1)[-len(self.shape):]
        self._ptr, self._contiguous = ptr, contiguous

    dim = lambda self: len(self.shape)
    stride = lambda self, i: self._stride[i]
    numel = lambda self: self.shape[0] * (self.shape[1] if len(self.shape) > 1 else 1)
    is_contiguous = lambda self: self._contiguous
    data_ptr = lambda self: self._ptr


class Torch:
    uint8, int32 = UINT8, INT32

    def __init__(self):
        self.allocated = []
        self.cuda = types.SimpleNamespace(
            current_device=lambda: 0,
            current_stream=lambda: types.SimpleNamespace(cuda_stream=STREAM[1]))

    def empty(self, n, dtype, device):
        self.allocated.append((dtype, n))
        return Tensor(dtype, n, 0xA000 + 0x100 * len(self.allocated))


def plain(a):
    if isinstance(a, ctypes.c_void_p):
        return ("vp", a.value)
    if isinstance(a, ctypes.Array):
        a[:] = range(len(a))
        return (type(a)._type_.__name__, len(a))
    return "out" if hasattr(a, "_obj") else a


class Lib:
    def __init__(self, need=0):
        self.need, self.calls = need, []

    def __getattr__(self, name):
        def entry(*args):
            if name.endswith("_workspace"):
                args[-1]._obj.value = self.need
            self.calls.append((name, tuple(plain(a) for a in args)))
            return 0
        return entry


@pytest.fixture
def dev(le, monkeypatch):
    assert le.layout("vandrs", (4, 2, 8), 1000)[0] == BS
    monkeypatch.setattr(le.device, "lib", Lib())
    monkeypatch.setattr(le.device, "torch", Torch())
    return le.device


# One batch: vandrs(4,2,8), 3 objects of 1,000 bytes in rows of 1,024, blocks
# of 256 bytes, parity rows of 512.
BS, NOBJ, SIZE, HEAD = 256, 3, 1000, 32
BATCH = ("vandrs", (4, 2, 8))
PREFIX = (2, 4, 2, 8, 0x1000, 1024, SIZE, NOBJ, 0x2000, 512)
PTR = {"flags": 0x3000, "lost": 0x3100, "unhealed": 0x3200, "report": 0x3300, "totals": 0x3400}
WS = (0x4000, 4096)
CAP = 256 << 20


def query(name):
    return (f"leoec_{name}_dev_workspace", (2, 4, 2, 8, SIZE, NOBJ, "out"))


def arenas():
    return Tensor(UINT8, (NOBJ, 1024), 0x1000), SIZE, Tensor(UINT8, (NOBJ, 512), 0x2000)


def words(name, n=None, dtype=INT32):
    return Tensor(dtype, (2 if name == "totals" else NOBJ) if n is None else n, PTR[name])


# call: (the words it takes in order of allocation, the ones the caller must
# give, the order in which they are checked, the library calls with every
# buffer given, what it returns)
CALLS = {
    "verify": (("flags",), (), ("flags",),
               [query("verify"), ("leoec_verify_dev", PREFIX + (0x3000,) + WS + (STREAM,))], "flags"),
    "heal": (("unhealed",), ("lost",), ("lost", "unhealed"),
             [("leoec_heal_dev", PREFIX + (0x3100, 0x3200, STREAM))], "unhealed"),
    "locate": (("lost",), (), ("lost",),
               [("leoec_locate_dev", PREFIX + (0x3100, STREAM))], "lost"),
    "locate_ws": (("lost",), (), ("lost",),
                  [query("locate_ws"), ("leoec_locate_ws_dev", PREFIX + (0x3100,) + WS + (STREAM,))], "lost"),
    "locate_gfw": (("lost",), (), ("lost",),
                   [query("locate_gfw"), ("leoec_locate_gfw_dev", PREFIX + (0x3100,) + WS + (STREAM,))],
                   "lost"),
    "scrub": (("report", "totals"), (), ("report", "totals"),
              [query("scrub"), ("leoec_scrub_dev", PREFIX + (0x3300, 0x3400) + WS + (STREAM,))],
              ("report", "totals")),
    "scrub_ws": (("report", "totals"), (), ("report", "totals"),
                 [query("scrub_ws"), ("leoec_scrub_ws_dev", PREFIX + (0x3300, 0x3400) + WS + (STREAM,))],
                 ("report", "totals")),
    "scrub_gfw": (("report", "totals"), (), ("report", "totals"),
                  [query("scrub_gfw"), ("leoec_scrub_gfw_dev", PREFIX + (0x3300, 0x3400) + WS + (STREAM,))],
                  ("report", "totals")),
    "heal_ws": (("unhealed", "totals"), ("lost",), ("lost", "unhealed", "totals"),
                [query("heal_ws"), ("leoec_heal_ws_dev", PREFIX + (0x3100, 0x3200, 0x3400) + WS + (STREAM,))],
                ("unhealed", "totals")),
}
ENCODE = ("verify", "locate_ws", "locate_gfw")      # a capped encode region, none for a query of 0
FIXED = ("scrub", "heal_ws")                        # the query's bytes
HEADED = ("scrub_ws", "scrub_gfw")                  # the header, then a capped encode region
WORKSPACE = ENCODE + FIXED + HEADED
# (query, bytes allocated): above the cap, below it, below m bs = 512, 0; HEADED: and the header alone
ALLOCATED = {
    ENCODE: [(CAP + 1, CAP), (4096, 4096), (100, 512), (0, None)],
    FIXED: [(CAP + 1, CAP + 1), (4096, 4096), (100, 100), (0, 0)],
    HEADED: [(HEAD + CAP + 1, HEAD + CAP), (HEAD + 4096, HEAD + 4096), (HEAD + 100, HEAD + 512),
             (HEAD, HEAD), (0, HEAD + 512)],
}
STREAM_ERROR = {
    "verify": "verify on an explicit stream needs an explicit workspace (4096 B for one pass, at least 512 B)",
    "locate_ws": "locate_ws on an explicit stream needs an explicit workspace "
                 "(4096 B for one pass, at least 512 B)",
    "locate_gfw": "locate_gfw on an explicit stream needs an explicit workspace "
                  "(4096 B for one pass, at least 512 B)",
    "scrub": "scrub on an explicit stream needs an explicit workspace (4096 B)",
    "scrub_ws": "scrub_ws on an explicit stream needs an explicit workspace (4096 B for one pass)",
    "scrub_gfw": "scrub_gfw on an explicit stream needs an explicit workspace (4096 B for one pass)",
    "heal_ws": "heal_ws on an explicit stream needs an explicit workspace (4096 B)",
}


def kwargs(name, given=True, workspace=True):
    """The call's keyword arguments: the words the caller must give, and with
    `given` every other buffer."""
    takes, must, _, _, _ = CALLS[name]
    kw = {w: words(w) for w in must + (takes if given else ())}
    if given and workspace and name in WORKSPACE:
        kw["workspace"] = Tensor(UINT8, WS[1], WS[0])
    return kw


def returned(name, out, kw):
    ret = CALLS[name][4]
    if isinstance(ret, tuple):
        return all(o is kw[r] for o, r in zip(out, ret)) and len(out) == len(ret)
    return out is kw[ret]


@pytest.mark.parametrize("name", CALLS)
def test_call_sequence_with_every_buffer_given(dev, name):
    dev.lib.need = 4096
    kw = kwargs(name)
    out = getattr(dev, name)(*BATCH, *arenas(), **kw)
    assert dev.lib.calls == CALLS[name][3]
    assert dev.torch.allocated == [] and returned(name, out, kw)


@pytest.mark.parametrize("name", CALLS)
def test_explicit_stream_is_passed_on(dev, name):
    dev.lib.need = 4096
    getattr(dev, name)(*BATCH, *arenas(), stream=0x77, **kwargs(name))
    entry, args = CALLS[name][3][-1]
    assert dev.lib.calls[-1] == (entry, args[:-1] + (("vp", 0x77),))


@pytest.mark.parametrize("name,need,nbytes", [(name, need, nbytes) for group, rows in ALLOCATED.items()
                                              for name in group for need, nbytes in rows])
def test_allocations_with_nothing_given(dev, name, need, nbytes):
    dev.lib.need = need
    takes, must, _, calls, _ = CALLS[name]
    out = getattr(dev, name)(*BATCH, *arenas(), **kwargs(name, given=False))
    want = [(INT32, 2 if w == "totals" else NOBJ) for w in takes]
    assert dev.torch.allocated == want + ([(UINT8, nbytes)] if nbytes is not None else [])
    # the tensors allocated are the ones passed on, in that order, and returned
    ptrs = [0xA100 + 0x100 * i for i in range(len(want) + 1)]
    entry, args = calls[-1]
    tail = tuple(PTR[w] for w in must) + tuple(ptrs[:len(want)])
    tail += (ptrs[len(want)], nbytes) if nbytes is not None else (None, 0)
    assert dev.lib.calls == [calls[0], (entry, PREFIX + tail + (STREAM,))]
    assert [t.data_ptr() for t in (out if isinstance(out, tuple) else (out,))] == ptrs[:len(want)]


@pytest.mark.parametrize("name", ("heal", "locate"))
def test_allocations_of_the_calls_without_workspace(dev, name):
    takes, must, _, calls, _ = CALLS[name]
    out = getattr(dev, name)(*BATCH, *arenas(), **kwargs(name, given=False))
    assert dev.torch.allocated == [(INT32, NOBJ)] and out.data_ptr() == 0xA100
    entry, args = calls[-1]
    assert dev.lib.calls == [(entry, PREFIX + tuple(PTR[w] for w in must) + (0xA100, STREAM))]


@pytest.mark.parametrize("name", STREAM_ERROR)
def test_explicit_stream_without_workspace(dev, name):
    dev.lib.need = 4096
    with pytest.raises(ValueError) as e:
        getattr(dev, name)(*BATCH, *arenas(), stream=0x77, **kwargs(name, workspace=False))
    assert str(e.value) == STREAM_ERROR[name]
    assert dev.lib.calls == CALLS[name][3][:1]  # the query alone


@pytest.mark.parametrize("name", ENCODE)
def test_explicit_stream_with_a_query_of_zero_needs_no_workspace(dev, name):
    getattr(dev, name)(*BATCH, *arenas(), stream=0x77, **kwargs(name, workspace=False))
    entry, args = CALLS[name][3][-1]
    assert dev.lib.calls[-1] == (entry, args[:-3] + (None, 0, ("vp", 0x77)))


@pytest.mark.parametrize("name,bad", [(name, bad) for name in CALLS for bad in CALLS[name][2]])
def test_bad_words(dev, name, bad):
    """A words tensor of the wrong dtype, then one too short, the other
    buffers not given: raised after every allocation of words and the checks
    of the words before it, before any library call."""
    takes, must, order, _, _ = CALLS[name]
    need = 2 if bad == "totals" else NOBJ
    for tensor, text in ((words(bad, dtype=UINT8), f"{bad}: contiguous 1-D int32 device tensor expected"),
                         (words(bad, n=need - 1), f"{bad}: {need - 1} words, {need} needed")):
        dev.lib.calls.clear()
        dev.torch.allocated.clear()
        kw = dict(kwargs(name, given=False), **{bad: tensor})
        with pytest.raises(ValueError) as e:
            getattr(dev, name)(*BATCH, *arenas(), **kw)
        assert str(e.value) == text
        assert dev.lib.calls == []
        assert dev.torch.allocated == [(INT32, 2 if w == "totals" else NOBJ) for w in takes if w != bad]


@pytest.mark.parametrize("name", ("scrub", "scrub_ws", "scrub_gfw", "heal_ws"))
def test_words_are_checked_in_order(dev, name):
    """Two bad tensors: the error is the first one's in the order of checks."""
    order = CALLS[name][2]
    kw = dict(kwargs(name), **{w: words(w, dtype=UINT8) for w in order[-2:]})
    with pytest.raises(ValueError) as e:
        getattr(dev, name)(*BATCH, *arenas(), **kw)
    assert str(e.value) == f"{order[-2]}: contiguous 1-D int32 device tensor expected"


@pytest.mark.parametrize("name", WORKSPACE)
def test_bad_workspace(dev, name):
    """Not contiguous, then not uint8: raised after the query, before the call."""
    dev.lib.need = 4096
    for ws in (Tensor(UINT8, WS[1], WS[0], contiguous=False), Tensor(INT32, WS[1], WS[0])):
        dev.lib.calls.clear()
        with pytest.raises(ValueError) as e:
            getattr(dev, name)(*BATCH, *arenas(), **dict(kwargs(name), workspace=ws))
        assert str(e.value) == "workspace: contiguous uint8 device tensor expected"
        assert dev.lib.calls == CALLS[name][3][:1]


def test_bad_rows_come_first(dev):
    """_batch's checks precede everything: nothing allocated, nothing called."""
    objs, size, par = arenas()
    for name in CALLS:
        with pytest.raises(ValueError) as e:
            getattr(dev, name)(*BATCH, objs, size, Tensor(UINT8, (NOBJ, 511), 0x2000),
                               **kwargs(name, given=False))
        assert str(e.value) == "parity: rows of 511 B, 512 B needed"
    assert dev.lib.calls == [] and dev.torch.allocated == []


@pytest.mark.parametrize("name", ("verify", "locate_ws", "locate_gfw", "scrub", "scrub_ws", "scrub_gfw",
                                  "heal_ws"))
def test_workspace_queries(dev, name):
    dev.lib.need = 12345
    assert getattr(dev, name + "_workspace")(*BATCH, SIZE, NOBJ) == 12345
    assert dev.lib.calls == [query(name)]


ROWS = (2, 5, 3, 8)  # vandrs(5,3,8): (m - 1) k = 10 ratios, rows of ceil(5 * 8 / 32) = 2 words
PAIRS = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11], [12, 13], [14, 15]]


@pytest.mark.parametrize("name,args,call,want", [
    ("locate_rows", (), ROWS + (("c_uint", 10), 10), [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]),
    ("locate_wrows", (), ROWS + (("c_uint", 10), 10), [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9]]),
    ("scrub_bitrows", (6,), ROWS + (6, ("c_int", 5), ("c_uint", 16), 16), ([0, 1, 2, 3, 4], PAIRS)),
    ("heal_bitrows", (0x41, 1), ROWS + (0x41, 1, ("c_int", 5), ("c_uint", 16), 16), ([0, 1, 2, 3, 4], PAIRS)),
    ("scrub_wrows", (6,), ROWS + (6, ("c_int", 5), ("c_uint", 5), 5), ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4])),
    ("heal_wrows", (0x41, 1), ROWS + (0x41, 1, ("c_int", 5), ("c_uint", 5), 5),
     ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4])),
])
def test_rows(dev, name, args, call, want):
    assert getattr(dev, name)("vandrs", (5, 3, 8), *args) == want
    assert dev.lib.calls == [("leoec_" + name, call)]
