"""leoec_read_dev on the GPU: a byte range of every object of a degraded batch
read into `out`, the bytes leoec_decode_dev would leave in objs, without
rebuilding a block (include/leoec.h).

Five objects per batch in gpu_helpers' poisoned arenas with guard rows; every
erased block, data and coding, is overwritten with POISON before the call, and
every byte of objs, parity and out is compared after it (read_helpers: objs and
parity still their poisoned snapshots, out the object's bytes at [lead,
lead + length) of every row and the fill everywhere else).  The ranges
(update_helpers.ranges) are the smallest shapes that can go wrong: head and
tail lanes, single bytes inside w = 16 / 32 words, block and packet boundaries,
whole packets and blocks, the ragged last block, the kernels' tile seams,
several blocks with partial ends.  Every range runs the erased sets A (the first
blocks of the range, up to m) and B (the range's last block and coding block 0);
ranges of three blocks or more also C (intact, lost, intact, lost); D (nothing
erased, and coding ids only) is a pure copy on four ranges.

Families: update_helpers.FAMILIES (vandrs(20,4,8) and vandrs(30,4,16): two
gf_read launches) and liberation(28,2,29) (two bit_read launches).  Sizes:
k B - 17 and a small one whose last data block is empty.

The launcher's chunk seam (LEOEC_READ_CHUNK) is test_read_forms.py, in the
measurement build's own process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_helpers as H
import read_helpers as R
import stream_helpers as S
import update_helpers as U
from test_pending_hip_error import _check_calls, hip, planted  # noqa: F401  (hip: a fixture)


@pytest.fixture(scope="module", params=R.FAMILIES, ids=R.family_id)
def family(request):
    return request.param


def test_case_table(le, family):
    """A condition on the inputs (no GPU), through the library's own layout:
    on every range of both sizes A and B each erase a data block the range
    meets and leave k intact ids, and C applies to at least one range."""
    cls, k, m, w, B = family
    for size in R.sizes(family):
        bs, _ = le.layout(cls, (k, m, w), size)
        rs = R.ranges(family, size, bs)
        assert len(rs) >= 10
        with_c = 0
        for off, length in rs:
            j0, j1 = R.blocks_of(off, length, bs)
            sets = R.erased_sets(family, off, length, bs)
            assert "A" in sets and (m < 2 or "B" in sets)
            for name, erased in sets.items():
                assert len(set(erased)) == len(erased) <= m, (name, erased)
                lost = [e for e in erased if e < k]
                assert lost and all(j0 <= e <= j1 for e in lost), (name, off, length, erased)
                assert all(e * bs < size for e in lost)
            assert sets["A"][0] == j0 and ("B" not in sets or sets["B"] == [j1, k])
            with_c += "C" in sets
        assert with_c >= 1, (family, size)
    assert bs * k >= size and H.block_valids(k, bs, size)[-1] == 0  # the small size: an empty last block


@pytest.mark.gpu
def test_device_read_ranges(gpu, le, oracle, family):
    errors = []
    for size in R.sizes(family):
        case = H.edge_case(le, oracle, family[:4], size)
        for off, length in R.ranges(family, size, case.bs):
            for name, erased in R.erased_sets(family, off, length, case.bs).items():
                errors += R.run_read(gpu, le, case, erased, off, length, name)
    assert not errors, "\n".join(e[:600] for e in errors[:10])


@pytest.mark.gpu
def test_nothing_lost_is_a_copy(gpu, le, oracle, family):
    """D: no id erased, and the coding ids only: no data block is lost, the
    range is one copy run and the poisoned coding blocks are never read."""
    cls, k, m, w, B = family
    errors = []
    for size in R.sizes(family):
        case = H.edge_case(le, oracle, family[:4], size)
        for off, length in R.copy_ranges(size, case.bs):
            errors += R.run_read(gpu, le, case, [], off, length, "D none")
            errors += R.run_read(gpu, le, case, list(range(k, k + m)), off, length, "D coding")
    assert not errors, "\n".join(e[:600] for e in errors[:10])


DECODE_FAMILIES = [("vandrs", 10, 4, 8, 8704), ("isars", 10, 4, 8, 8704), ("cauchyrs", 10, 4, 8, 4352 * 8),
                   ("liberation", 10, 2, 11, 2176 * 11), ("vandrs", 10, 4, 16, 8704)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", DECODE_FAMILIES, ids=R.family_id)
def test_read_is_decode_dev_on_a_damaged_stripe(gpu, le, oracle, fam):
    """From random parity no object is a codeword: out must equal the range of
    the rows leoec_decode_dev leaves on a clone with the same erased list,
    which pins the survivor choice (another set of k survivors gives other
    bytes on a damaged stripe)."""
    assert fam in R.FAMILIES
    cls, k, m, w, B = fam
    case = H.edge_case(le, oracle, fam[:4], R.sizes(fam)[0])
    g, n, bs = case.guard, case.n, case.bs
    rnd = U.random_parity(case)
    off, length = bs - 5, 2 * bs + 12  # three blocks, partial ends
    differs = 0
    for erased in ([0, 1, 2, 3][:m], [2, k], [1, k + m - 1], [0, k, k + 1][:m]):
        work, par = R.poisoned(gpu, case, rnd, erased)
        dec, dec_par = work.clone(), par.clone()
        out = le.device.read(cls, case.params, work[g:g + n], case.size, par[1:1 + n], erased, off, length)
        le.device.decode(cls, case.params, dec[g:g + n], case.size, dec_par[1:1 + n], erased)
        gpu.cuda.synchronize()
        lead = off % 16
        assert out.shape == (n, (lead + length + 15) // 16 * 16)
        want = dec[g:g + n, off:off + length]
        assert gpu.equal(out[:, lead:lead + length], want), (case.ident(), erased)
        differs += not np.array_equal(want.cpu().numpy(), case.rows[:, off:off + length])
    assert differs  # the stripe is damaged: decode does not give the object back


RAGGED_FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 10, 4, 16, 8704), ("vandrs", 6, 3, 32, 8704),
                   ("cauchyrs", 10, 4, 8, 4352 * 8), ("liberation", 4, 2, 7, 2176 * 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", RAGGED_FAMILIES, ids=R.family_id)
def test_the_ragged_survivor(gpu, le, oracle, fam):
    """Block 0 lost at the large size, the range on columns that lie past the
    last data block's valid bytes (B - 17): the survivor's lanes there are
    clipped and zero-filled.  The bytes behind every object are random
    non-zero, so a lane loaded whole shows.  (Implied by the ranges above;
    named here.)"""
    cls, k, m, w, B = fam
    case = H.edge_case(le, oracle, fam[:4], R.sizes(fam)[0])
    bs = case.bs
    assert H.block_valids(k, bs, case.size)[-1] == bs - 17
    errors = []
    for off, length in ((bs - 40, 40), (bs - 17, 17), (bs - 18, 2), (bs - 1, 1)):
        errors += R.run_read(gpu, le, case, [0], off, length, "ragged survivor")
    assert not errors, "\n".join(e[:600] for e in errors)


def _stream_case(le, oracle, family):
    case = H.edge_case(le, oracle, family[:4], S.edge_size(family))
    off = case.bs - 5  # intact, lost, intact, lost with C's set (k = 4: to the object's end)
    return case, off, min(3 * case.bs + 12, case.size - off), [1, 3]


STREAM_FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 20, 4, 8, 8704), ("vandrs", 6, 3, 32, 8704),
                   ("cauchyrs", 10, 4, 8, 4352 * 8), ("liberation", 10, 2, 11, 2176 * 11)]


@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES, ids=R.family_id)
def test_captured_read(gpu, le, oracle, fam):
    """One read captured into a graph (after a plain call) and replayed on
    fresh data and on a second batch's bytes (the objects rotated by one) in
    the same buffers: the capture itself writes nothing, every replay reads
    the batch then in the buffers."""
    assert fam in R.FAMILIES
    case, off, length, erased = _stream_case(le, oracle, fam)
    g, n = case.guard, case.n
    first = R.poisoned(gpu, case, case.parity, erased)
    second = (S.rolled(first[0], g, n), S.rolled(first[1], 1, n))
    rows2 = case.rows[S.rotation(n)]
    work, par = first[0].clone(), first[1].clone()
    out_fill = R.out_arena(gpu, case, off, length)
    out = out_fill.clone()
    src = [first]

    def refill():
        work.copy_(src[0][0])
        par.copy_(src[0][1])
        out.copy_(out_fill)

    ctx = f"captured read {case.ident()} [{off}, +{length})"
    cap = S.Captured(gpu, lambda: le.device.read(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n],
                                                 erased, off, length, out=out[1:1 + n]),
                     refill, lambda: S._diffs(gpu, [(out, out_fill, 1, f"{ctx}: out")]))
    errors = cap.errors
    for r, (batch, rows) in enumerate(((first, case.rows), (second, rows2), (first, case.rows))):
        src[0] = batch
        refill()
        cap.replay()
        errors += S._diffs(gpu, [(out, R.expected_out(gpu, case, rows, off, length), 1, f"{ctx} replay {r}: out"),
                                 (work, batch[0], g, f"{ctx} replay {r}: objs"),
                                 (par, batch[1], 1, f"{ctx} replay {r}: parity")])
    assert not errors, "\n".join(e[:600] for e in errors[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("fam", STREAM_FAMILIES[1:2] + STREAM_FAMILIES[3:4], ids=R.family_id)
def test_read_on_a_side_stream(gpu, le, oracle, fam):
    """The read on a non-blocking side stream behind a large fill and the
    copies that bring the batch in, nothing but the stream's own
    synchronisation at the end: a launch on another stream would read the
    zeroed buffers."""
    case, off, length, erased = _stream_case(le, oracle, fam)
    g, n = case.guard, case.n
    work_snap, par_snap = R.poisoned(gpu, case, case.parity, erased)
    out_fill = R.out_arena(gpu, case, off, length)
    le.device.read(case.cls, case.params, work_snap.clone()[g:g + n], case.size, par_snap.clone()[1:1 + n],
                   erased, off, length, out=out_fill.clone()[1:1 + n])  # the plain call: the code object, the rows
    work, par, out = gpu.zeros_like(work_snap), gpu.zeros_like(par_snap), gpu.zeros_like(out_fill)
    scratch = gpu.empty((S.WINDOW_BYTES,), dtype=gpu.uint8, device="cuda")
    side = gpu.cuda.Stream()
    assert side.cuda_stream != 0
    gpu.cuda.synchronize()
    with gpu.cuda.stream(side):
        scratch.fill_(0x11)
        work.copy_(work_snap)
        par.copy_(par_snap)
        out.copy_(out_fill)
        le.device.read(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], erased, off, length,
                       out=out[1:1 + n])
    side.synchronize()
    ctx = f"side-stream read {case.ident()}"
    errors = S._diffs(gpu, [(out, R.expected_out(gpu, case, case.rows, off, length), 1, f"{ctx}: out"),
                            (work, work_snap, g, f"{ctx}: objs"), (par, par_snap, 1, f"{ctx}: parity")])
    assert not errors, "\n".join(e[:600] for e in errors)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", [("vandrs", 20, 4, 8, 8704), ("vandrs", 10, 4, 16, 8704),
                                 ("cauchyrs", 4, 4, 17, 8704 * 17)], ids=R.family_id)
def test_read_with_a_pending_hip_error(gpu, le, oracle, hip, fam):  # noqa: F811
    """hipErrorInvalidDevice pending on the calling thread: every launch of the
    call (copy runs, and two launches per lost block for k = 20) succeeds, the
    status is LEOEC_OK, the bytes are right and the caller's error is still in
    the slot afterwards."""
    case, off, length, erased = _stream_case(le, oracle, fam)
    with planted(gpu, le, hip, "leoec_read_dev") as calls:
        errors = R.run_read(gpu, le, case, erased, off, length, "C")
    _check_calls(calls, "leoec_read_dev")
    assert not errors, "\n".join(e[:600] for e in errors)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_wide_strides_in_own_process(gpu, tmp_path):
    """Three objects whose objs, parity and out rows lie 2^32 + 48 bytes apart
    (read_wide_child.py, a fresh process that holds the 17 GB allocation):
    o * stride crosses 2^32 and 2^33."""
    import read_wide_child as C
    gpu.cuda.empty_cache()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    log = str(tmp_path / "read_wide_child.log")
    with open(log, "w") as fh:
        rc = subprocess.call([sys.executable, "-u", os.path.abspath(C.__file__)], cwd=root, env=env,
                             stdout=fh, stderr=subprocess.STDOUT, timeout=240)
    with open(log) as fh:
        text = fh.read()
    assert rc == 0, f"rc {rc}, {log}:\n{text[-4000:]}"
    assert text.strip().splitlines()[-1] == f"ok: {len(C.FAMILIES)} families", text[-2000:]
