"""leoec_heal_ws_dev on the device (product library): heal_helpers.run_heal's
standard (poisoned arenas with guard rows, every byte of every buffer
compared, unhealed between sentinels, lost unchanged), the totals, the
workspace's tail, and objs / parity / unhealed byte for byte against a
leoec_heal_dev run over clones of the same damaged arenas
(heal_ws_helpers.run_heal_ws)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_helpers as H
import heal_helpers as HH
import heal_ws_helpers as X
import pending_helpers as PE
import stream_helpers as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=HH.FAMILIES, ids=HH.family_id)
def family(request):
    return request.param


def test_families_are_served(le):
    assert len(HH.FAMILIES) == 15
    for cls, k, m, w, B in HH.FAMILIES:
        assert X.served(cls, k, m, w)
        assert le.device.heal_ws_workspace(cls, (k, m, w), k * B - 1, HH.EDGE_N) == X.head(HH.EDGE_N)


@pytest.mark.gpu
def test_device_heal_ws_edge_masks(gpu, le, oracle, family):
    """edge_masks at k B - 1, 16 w (k - 2) + 5 and k B: ragged and empty
    outputs, full survivors, a word cut in the middle, both unrecoverable
    kinds; then the same batch with the last two objects left out."""
    cls, k, m, w, B = family
    masks = HH.edge_masks(k, m)
    errors = []
    for size in X.sizes(family):
        case = H.edge_case(le, oracle, family[:4], size, n=HH.EDGE_N)
        errors += X.run_heal_ws(gpu, le, case, masks)
        if size == X.sizes(family)[0]:
            errors += X.run_heal_ws(gpu, le, case, masks, nobj=HH.EDGE_N - 2)
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


# every mask of 0..m+1 bits, one object each, blocks of 16 w 2 bytes;
# vandrs(6,5,8): the 1,024 masks of 0..m bits
EVERY = [("vandrs", 4, 2, 16), ("vandrs", 6, 3, 32), ("cauchyrs", 6, 3, 4), ("liberation", 4, 2, 7),
         ("vandrs", 4, 2, 8), ("vandrs", 6, 5, 8)]


def every_masks(cfg):
    cls, k, m, w = cfg
    return HH.all_masks(k, m, 0, m if cfg == ("vandrs", 6, 5, 8) else m + 1)


def test_every_mask_batches_are_what_they_say(le):
    assert len(every_masks(("vandrs", 6, 5, 8))) == 1024
    for cfg in EVERY:
        cls, k, m, w = cfg
        masks = every_masks(cfg)
        assert len(set(masks)) == len(masks) and masks[0] == 0
        assert le.layout(cls, (k, m, w), k * 32 * w - 1)[0] == 32 * w


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", EVERY, ids=str)
def test_device_heal_ws_every_mask(gpu, le, oracle, cfg):
    """Every record and every rank of the code's table: one object per mask."""
    cls, k, m, w = cfg
    masks = every_masks(cfg)
    case = X.mask_case(le, oracle, cfg, 32 * w, masks)
    errors = X.run_heal_ws(gpu, le, case, masks)
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [("vandrs", 30, 2, 16), ("vandrs", 30, 2, 8), ("cauchyrs", 30, 2, 5)],
                         ids=str)
def test_device_heal_ws_32_ids(gpu, le, oracle, cfg):
    """k + m = 32: bit 31 is block 31 like any other."""
    cls, k, m, w = cfg
    masks = [HH.bits([31]), HH.bits([30, 31]), HH.bits([0, 31]), HH.bits([0]), HH.bits([29, 30, 31]), 0]
    assert masks[0] == 0x80000000 and not HH.recoverable(masks[4], k, m)
    case = X.mask_case(le, oracle, cfg, 32 * w, masks)
    errors = X.run_heal_ws(gpu, le, case, masks)
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


# one word family and one packet family with more than one tile a block / a packet
LARGE = [("vandrs", 2, 2, 16, 4352), ("cauchyrs", 2, 2, 4, 1088 * 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", LARGE, ids=HH.family_id)
def test_device_heal_ws_batch_larger_than_the_grid(gpu, le, oracle, fam):
    """Every object loses two blocks, masks alternating, with objects x m x
    tiles at least twice the rebuild grid (compute units x resident
    workgroups): every workgroup takes a second item (`item += gridDim.x`),
    so an accumulator kept from the first would show."""
    cls, k, m, w, B = fam
    cus = gpu.cuda.get_device_properties(gpu.cuda.current_device()).multi_processor_count
    tile_of = (B // w) if HH.bitsliced(cls) else B
    tiles = -(-tile_of // (X.TILE_BIT if HH.bitsliced(cls) else X.TILE_GFW))
    assert tiles == 2
    grid = cus * X.resident(cls, w)
    n = -(-2 * grid // (m * tiles))
    case = H.EdgeCase(le, oracle, fam[:4], k * B - 1, n)
    assert case.bs == B and n * m * tiles >= 2 * grid
    pairs = [HH.bits(c) for c in ((0, 1), (1, 2), (0, 3), (2, 3), (1, 3), (0, 2))]
    masks = [pairs[o % len(pairs)] for o in range(n)]
    errors = X.run_heal_ws(gpu, le, case, masks)
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


# ---------------------------------------------------------------------------
# Capture and a side stream (stream_helpers' pattern).

STREAM_FAMILIES = [("vandrs", 10, 4, 16, 8704), ("cauchyrs", 6, 3, 4, 4352 * 4)]


class _Batch:
    """The arenas and the call's buffers of one case, refilled from a damaged
    pair of arenas and their masks."""

    def __init__(self, gpu, le, case):
        self.gpu, self.le, self.case = gpu, le, case
        snap, par_snap = case.dev(gpu)
        self.work, self.par = gpu.zeros_like(snap), gpu.zeros_like(par_snap)
        self.buf = X.Buffers(gpu, [0] * case.n)

    def refill(self, src, masks):
        self.work.copy_(src[0])
        self.par.copy_(src[1])
        self.buf.lost_host = np.array(masks, dtype=np.uint32).view(np.int32)
        self.buf.lost.copy_(self.gpu.from_numpy(self.buf.lost_host.copy()))
        self.buf.reset(self.gpu)

    def call(self, stream=None):
        X.call(self.le, self.case, self.work, self.par, self.buf, stream=stream)

    def untouched(self, src):
        errors = T._diffs(self.gpu, [(self.work, src[0], self.case.guard, "objs"), (self.par, src[1], 1, "parity")])
        n = self.case.n
        if X.u32(self.buf.unhealed)[1:-1] != [HH.PREFILL] * n:
            errors.append("unhealed written")
        if X.u32(self.buf.totals)[1:3] != [X.TOTALS_PREFILL] * 2:
            errors.append("totals written")
        return errors

    def check(self, want, masks, ctx):
        errors = T._diffs(self.gpu, [(self.work, want[0], self.case.guard, f"{ctx}: objs"),
                                     (self.par, want[1], 1, f"{ctx}: parity")])
        return errors + X.check_words(self.gpu, self.case, masks, self.buf, self.case.n, ctx)


def _stream_batches(gpu, le, oracle, fam):
    cls, k, m, w, B = fam
    case = H.edge_case(le, oracle, fam[:4], X.sizes(fam)[0], n=HH.EDGE_N)
    first = HH.edge_masks(k, m)
    second = list(reversed(first))
    return case, [(masks, X.damaged(gpu, case, masks)) for masks in (first, second)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES, ids=HH.family_id)
def test_device_heal_ws_captured(gpu, le, oracle, fam):
    """After one plain call (the table, the code objects) the call is captured
    into a graph, writes nothing during the capture, and three replays over
    fresh damage (the edge masks, the same reversed, the edge masks) give each
    batch's bytes, unhealed and totals."""
    case, batches = _stream_batches(gpu, le, oracle, fam)
    b = _Batch(gpu, le, case)
    masks0, (w0, p0, _, _) = batches[0]
    cap = T.Captured(gpu, b.call, lambda: b.refill((w0, p0), masks0), lambda: b.untouched((w0, p0)))
    errors = cap.errors
    for r, (masks, (work, par, want, par_want)) in enumerate((batches[0], batches[1], batches[0])):
        b.refill((work, par), masks)
        cap.replay()
        errors += b.check((want, par_want), masks, f"captured heal_ws {case.ident()} replay {r}")
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES, ids=HH.family_id)
def test_device_heal_ws_on_side_stream(gpu, le, oracle, fam):
    """Behind a large fill and the copies that bring the damaged batch in, on
    a non-blocking side stream, with nothing but that stream's own
    synchronisation afterwards (a plain call on the null stream comes first)."""
    case, batches = _stream_batches(gpu, le, oracle, fam)
    masks, (work, par, want, par_want) = batches[0]
    b = _Batch(gpu, le, case)
    b.refill((work, par), masks)
    b.call()
    gpu.cuda.synchronize()
    b.refill((gpu.zeros_like(work), gpu.zeros_like(par)), masks)
    scratch = gpu.empty((T.WINDOW_BYTES,), dtype=gpu.uint8, device="cuda")
    side = gpu.cuda.Stream()
    assert side.cuda_stream != 0 and side != gpu.cuda.default_stream()
    gpu.cuda.synchronize()  # the buffers above were filled on the null stream
    with gpu.cuda.stream(side):
        scratch.fill_(0x11)
        b.work.copy_(work)
        b.par.copy_(par)
        b.call(stream=side.cuda_stream)
    side.synchronize()
    errors = b.check((want, par_want), masks, f"side stream heal_ws {case.ident()}")
    assert not errors, "\n".join(e[:1500] for e in errors[:12])


# ---------------------------------------------------------------------------
# A HIP error pending on the calling thread (test_pending_hip_error.py's way:
# hipSetDevice(-1) through the library's own runtime handle, no torch call
# between planting and the clear).

@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES, ids=HH.family_id)
def test_device_heal_ws_with_pending_error(gpu, le, oracle, fam):
    """A first plain call, then one with hipErrorInvalidDevice pending on the
    thread: LEOEC_OK, the results right, the same code in the slot afterwards."""
    cls, k, m, w, B = fam
    case = H.edge_case(le, oracle, fam[:4], X.sizes(fam)[0], n=HH.EDGE_N)
    masks = HH.edge_masks(k, m)
    first = X.run_heal_ws(gpu, le, case, masks, reference=False)
    assert not first, "\n".join(first)
    calls = []
    with PE.planted(gpu, le, calls, "leoec_heal_ws_dev") as rt:
        errors = X.run_heal_ws(gpu, le, case, list(reversed(masks)), reference=False)
    assert calls == [(0, PE.HIP_ERROR_INVALID_DEVICE)], calls
    assert not errors, "\n".join(errors)
    assert rt.hipPeekAtLastError() == PE.HIP_SUCCESS


# ---------------------------------------------------------------------------
# Child processes: the table cache full; rows more than 4 GiB apart.

def _child(tmp_path, script, timeout):
    log = str(tmp_path / (script + ".log"))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    cmd = [sys.executable, "-u", os.path.join(ROOT, "tests", script)]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=ROOT, env=env, stdout=fh, stderr=subprocess.STDOUT, timeout=timeout)
    with open(log) as fh:
        text = fh.read()
    return rc, text, log


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_heal_ws_with_full_table_cache_in_own_process(gpu, tmp_path):
    """tests/heal_ws_table_cache_child.py in a fresh process: 16 word
    configurations healed first fill this call's table cache, the heal of a
    17th then counts on the device, takes leoec_heal_dev's own path and must
    still equal it byte for byte, totals included."""
    rc, text, log = _child(tmp_path, "heal_ws_table_cache_child.py", 280)
    assert rc == 0, f"heal_ws_table_cache_child.py failed (rc {rc}), {log}:\n{text[-4000:]}"
    assert "17th configuration healed" in text, text[-4000:]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_heal_ws_wide_strides_in_own_process(gpu, tmp_path):
    """tests/heal_ws_wide_child.py in a fresh process: three objects whose rows
    lie 2^32 + 48 bytes apart, one word family and one packet family."""
    rc, text, log = _child(tmp_path, "heal_ws_wide_child.py", 560)
    lines = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    if rc == 3:
        pytest.skip("the wide allocation cannot be made: " + text[-300:])
    assert rc == 0, f"heal_ws_wide_child.py failed (rc {rc}), {log}:\n{text[-4000:]}"
    cases = [x for x in lines if "case" in x]
    assert len(cases) == 2 and lines[-1].get("done") == 2, text[-4000:]
    assert all(not x["errors"] for x in cases), cases
