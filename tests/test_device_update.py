"""leoec_update_dev on the GPU: a byte range of every object of a stored batch
overwritten in place and the parity patched to match (include/leoec.h).

Five objects per batch in gpu_helpers' poisoned arenas with guard rows; every
byte of objs, parity and patch is compared after every call (update_helpers:
objs patched in numpy, parity = parity before ^ the oracle's encoding of the
delta D, the patch as it was, poison around its bytes).  Every range runs from
consistent parity, where the result is also the oracle's encoding of the new
object, and from random parity, which a re-encoding implementation fails; the
new bytes differ from the old in every byte of the range, so every store is
needed.  The ranges (update_helpers.ranges) are the smallest shapes that can go
wrong: head and tail lanes, single bytes inside w = 16 / 32 words, block and
packet boundaries, whole packets and blocks, the ragged last block, both
kernels' tile seams, several blocks with partial ends.

Families: gpu_helpers.EDGE_FAMILIES, vandrs(20,4,8), vandrs(6,5,8) and
vandrs(16,15,8) (coding rows in 2 and 4 launches: only the last stores the new
bytes), vandrs(30,4,16) (k + m = 34), cauchyrs(4,4,17) (68 bit-rows: 2 launches).  Sizes: k B - 17 and a small one whose
last data block is empty.

The launcher's chunk seam (LEOEC_UPDATE_CHUNK) is test_update_forms.py, in the
measurement build's own process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_helpers as H
import stream_helpers as S
import update_helpers as U
from test_pending_hip_error import _check_calls, hip, planted  # noqa: F401  (hip: a fixture)


@pytest.fixture(scope="module", params=U.FAMILIES, ids=U.family_id)
def family(request):
    return request.param


def test_case_table(le, family):
    """The table through the library's own layout (no GPU): the large size
    holds every range of the list, the small one has an empty last block."""
    cls, k, m, w, B = family
    big, small = U.sizes(family)
    bs, _ = le.layout(cls, (k, m, w), big)
    assert bs == B and H.block_valids(k, bs, big)[-1] == B - 17
    rs = U.ranges(family, big, bs)
    want = 14 + (2 if U.packet_class(cls) else 0)
    assert len(rs) == want, rs
    assert (0, big) in rs and (0, 1) in rs and (big - 1, 1) in rs and ((k - 1) * bs, bs - 17) in rs
    assert all((t - 1, 2) in rs for t in (1024, 4096))
    sbs, _ = le.layout(cls, (k, m, w), small)
    v = H.block_valids(k, sbs, small)
    assert v[-1] == 0 and 0 < v[-2] < sbs
    assert len(U.ranges(family, small, sbs)) >= 10


@pytest.mark.gpu
def test_device_update_ranges(gpu, le, oracle, family):
    errors = []
    for size in U.sizes(family):
        case = H.edge_case(le, oracle, family[:4], size)
        rnd = U.random_parity(case)
        for i, (off, length) in enumerate(U.ranges(family, size, case.bs)):
            errors += U.run_update(gpu, le, oracle, case, case.parity, off, length, "consistent")
            errors += U.run_update(gpu, le, oracle, case, rnd, off, length, "random")
            # consistent parity ^ the delta's encoding is the oracle's encoding of the new object
            o = i % case.n
            if not np.array_equal(case.parity[o] ^ U.delta_parity(oracle, case, off, length),
                                  U.oracle_parity_of_new(oracle, case, o, off, length)):
                errors.append(f"{case.ident()} [{off}, +{length}): the expected parity of object {o} "
                              "is not the oracle's encoding of the new object")
    assert not errors, "\n".join(e[:600] for e in errors[:10])


@pytest.mark.gpu
def test_delta_encoding_is_encode_dev(gpu, le, oracle, family):
    """The bytes XORed into the parity are leoec_encode_dev's coding blocks of
    D, byte for byte (three ranges of the large size)."""
    case = H.edge_case(le, oracle, family[:4], U.sizes(family)[0])
    rs = U.ranges(family, case.size, case.bs)
    for off, length in (rs[0], rs[8], rs[-1]):
        got = U.encode_dev_of_delta(gpu, le, case, off, length)
        assert np.array_equal(got, U.delta_parity(oracle, case, off, length)), (case.ident(), off, length)


@pytest.mark.gpu
def test_liberation_unreached_packets_keep_their_bytes(gpu, le, oracle):
    """A range inside one data packet leaves every coding packet whose bit-row
    does not select that packet equal to its bytes before the call (random
    parity): named here, implied by the full compare above."""
    fam = ("liberation", 4, 2, 7, 2176 * 7)
    cls, k, m, w, B = fam
    case = H.edge_case(le, oracle, fam[:4], U.sizes(fam)[0])
    bits = U.coding_bits(le, cls, k, m, w)
    ps, g, n = case.bs // w, case.guard, case.n
    rnd = U.random_parity(case)
    kept_total = 0
    for j, c in ((0, 0), (1, 3), (3, 6)):
        off, length = j * case.bs + c * ps + 37, 100  # inside packet c of block j
        snap, _ = case.dev(gpu)
        work, par = snap.clone(), U.parity_arena(gpu, case, rnd)
        patch = case.arena(gpu, U.patch_rows(case, off, length), U.PATCH_FILL)
        le.device.update(cls, case.params, work[g:g + n], case.size, par[1:1 + n], patch[1:1 + n], off, length)
        gpu.cuda.synchronize()
        got = par[1:1 + n].cpu().numpy()
        for q in range(m * w):
            reached = bool(bits[q, j * w + c])
            same = np.array_equal(got[:, q * ps:(q + 1) * ps], rnd[:, q * ps:(q + 1) * ps])
            assert same != reached, f"coding packet {q}, data packet ({j}, {c}): reached {reached}, unchanged {same}"
            kept_total += not reached
    assert kept_total > 0


def _stream_case(le, oracle, family):
    case = H.edge_case(le, oracle, family[:4], S.edge_size(family))
    off, length = case.bs - 5, 2 * case.bs + 12  # three blocks, partial ends
    return case, off, length


STREAM_FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 6, 5, 8, 8704), ("vandrs", 6, 3, 32, 8704),
                   ("cauchyrs", 10, 4, 8, 4352 * 8), ("liberation", 10, 2, 11, 2176 * 11)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES, ids=U.family_id)
def test_captured_update(gpu, le, oracle, fam):
    """One update captured into a graph (after a plain call) and replayed on a
    fresh patch: the capture itself writes nothing, every replay patches objs
    and parity with the patch then in the buffer."""
    assert fam in U.FAMILIES
    case, off, length = _stream_case(le, oracle, fam)
    g, n = case.guard, case.n
    snap, _ = case.dev(gpu)
    rnd = U.random_parity(case)
    par_snap = U.parity_arena(gpu, case, rnd)
    patches = [case.arena(gpu, U.patch_rows(case, off, length, salt), U.PATCH_FILL) for salt in (0, 1)]
    work, par, patch = snap.clone(), par_snap.clone(), patches[0].clone()
    src = [patches[0]]

    def refill():
        work.copy_(snap)
        par.copy_(par_snap)
        patch.copy_(src[0])

    ctx = f"captured update {case.ident()} [{off}, +{length})"
    cap = S.Captured(gpu, lambda: le.device.update(case.cls, case.params, work[g:g + n], case.size,
                                                   par[1:1 + n], patch[1:1 + n], off, length),
                     refill, lambda: S._diffs(gpu, [(work, snap, g, f"{ctx}: objs"),
                                                    (par, par_snap, 1, f"{ctx}: parity")]))
    errors = cap.errors
    for r, salt in enumerate((0, 1, 0)):
        src[0] = patches[salt]
        refill()
        cap.replay()
        want, par_want, _, _ = U.expected(gpu, oracle, case, rnd, off, length, salt)
        errors += S._diffs(gpu, [(work, want, g, f"{ctx} replay {r}: objs"),
                                 (par, par_want, 1, f"{ctx} replay {r}: parity"),
                                 (patch, patches[salt], 1, f"{ctx} replay {r}: patch")])
    assert not errors, "\n".join(e[:600] for e in errors[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES[:1] + STREAM_FAMILIES[3:4], ids=U.family_id)
def test_update_on_a_side_stream(gpu, le, oracle, fam):
    """The update on a non-blocking side stream behind a large fill and the
    copies that bring the batch in, nothing but the stream's own
    synchronisation at the end: a launch on another stream would read the
    zeroed buffers."""
    case, off, length = _stream_case(le, oracle, fam)
    g, n = case.guard, case.n
    snap, _ = case.dev(gpu)
    rnd = U.random_parity(case)
    par_snap = U.parity_arena(gpu, case, rnd)
    patch_snap = case.arena(gpu, U.patch_rows(case, off, length), U.PATCH_FILL)
    le.device.update(case.cls, case.params, snap.clone()[g:g + n], case.size, par_snap.clone()[1:1 + n],
                     patch_snap.clone()[1:1 + n], off, length)  # the plain call: the code object
    work, par, patch = gpu.zeros_like(snap), gpu.zeros_like(par_snap), gpu.zeros_like(patch_snap)
    scratch = gpu.empty((S.WINDOW_BYTES,), dtype=gpu.uint8, device="cuda")
    side = gpu.cuda.Stream()
    assert side.cuda_stream != 0
    gpu.cuda.synchronize()
    with gpu.cuda.stream(side):
        scratch.fill_(0x11)
        work.copy_(snap)
        par.copy_(par_snap)
        patch.copy_(patch_snap)
        le.device.update(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], patch[1:1 + n],
                         off, length)
    side.synchronize()
    want, par_want, _, _ = U.expected(gpu, oracle, case, rnd, off, length)
    ctx = f"side-stream update {case.ident()}"
    errors = S._diffs(gpu, [(work, want, g, f"{ctx}: objs"), (par, par_want, 1, f"{ctx}: parity"),
                            (patch, patch_snap, 1, f"{ctx}: patch")])
    assert not errors, "\n".join(e[:600] for e in errors)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [("vandrs", 6, 5, 8, 8704), ("vandrs", 10, 4, 16, 8704),
                                 ("cauchyrs", 4, 4, 17, 8704 * 17)], ids=U.family_id)
def test_update_with_a_pending_hip_error(gpu, le, oracle, hip, fam):  # noqa: F811
    """hipErrorInvalidDevice pending on the calling thread: every launch of the
    call (several per segment for m = 5 and for 68 bit-rows) succeeds, the
    status is LEOEC_OK, the bytes are right and the caller's error is still in
    the slot afterwards."""
    case, off, length = _stream_case(le, oracle, fam)
    with planted(gpu, le, hip, "leoec_update_dev") as calls:
        errors = U.run_update(gpu, le, oracle, case, U.random_parity(case), off, length, "random")
    _check_calls(calls, "leoec_update_dev")
    assert not errors, "\n".join(e[:600] for e in errors)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_wide_strides_in_own_process(gpu, tmp_path):
    """Three objects whose objs, parity and patch rows lie 2^32 + 48 bytes
    apart (update_wide_child.py, a fresh process that holds the 17 GB
    allocation): o * stride crosses 2^32 and 2^33."""
    import update_wide_child as C
    gpu.cuda.empty_cache()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    log = str(tmp_path / "update_wide_child.log")
    with open(log, "w") as fh:
        rc = subprocess.call([sys.executable, "-u", os.path.abspath(C.__file__)], cwd=root, env=env,
                             stdout=fh, stderr=subprocess.STDOUT, timeout=240)
    with open(log) as fh:
        text = fh.read()
    assert rc == 0, f"rc {rc}, {log}:\n{text[-4000:]}"
    assert text.strip().splitlines()[-1] == f"ok: {len(C.FAMILIES)} families", text[-2000:]
