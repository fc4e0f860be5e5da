"""Shared pieces of the leoec_read_dev tests (test_device_read.py,
test_read_forms.py, read_wide_child.py): the families, the erased sets of a
range, and one read call inside gpu_helpers' guarded arenas with every byte of
objs, parity and out compared afterwards.

Expected bytes.  Before the call every erased block, data and coding, is
overwritten with POISON in the work arenas, and those poisoned arenas are the
snapshots objs and parity must still equal afterwards: the call writes neither,
and a kernel that reads an erased block returns wrong bytes.  From consistent
parity (the oracle's blocks of the EdgeCase) out holds the object's own bytes,
case.rows[:, offset:offset + length], at [lead, lead + length) of every row and
the fill everywhere else, guard rows included."""
import numpy as np

import gpu_helpers as H
import update_helpers as U

# update_helpers.FAMILIES (k > 16 at w = 8 and w = 16: two gf_read launches, 16 + 4
# and 16 + 14 survivors), and 28 survivors of 1 + 29 argument words each: two
# bit_read launches
LIBERATION_WIDE = ("liberation", 28, 2, 29, 2176 * 29)
FAMILIES = U.FAMILIES + [LIBERATION_WIDE]
N = H.EDGE_N
OUT_FILL = H.POISON
family_id = U.family_id
sizes = U.sizes
ranges = U.ranges  # range_copy's and gf_read's tiles are 4 KiB, bit_read's 1 KiB: update's seams


def blocks_of(off, length, bs):
    """(j0, j1): the data blocks holding the range's first and last byte."""
    return off // bs, (off + length - 1) // bs


def erased_sets(family, off, length, bs):
    """{name: erased ids} of one range.  A: data blocks j0, j0 + 1, ... up to m
    of them that the range meets (later blocks of a long range stay intact: a
    copy run follows the rebuilt ones).  B (m >= 2): j1 and coding block 0, so
    the survivors use coding blocks from 1 up.  C (ranges of three blocks or
    more): j0 + 1, and j0 + 3 where the range reaches it: intact, lost, intact,
    lost."""
    cls, k, m, w, B = family
    j0, j1 = blocks_of(off, length, bs)
    sets = {"A": list(range(j0, min(j1, j0 + m - 1) + 1))}
    if m >= 2:
        sets["B"] = [j1, k]
    if j1 - j0 >= 2:
        sets["C"] = [j0 + 1] + ([j0 + 3] if j0 + 3 <= j1 and m >= 2 else [])
    return sets


def copy_ranges(size, bs):
    """The four ranges of the pure-copy cases: the object, one byte, across
    the first block boundary, the last block with a byte."""
    last = (size - 1) // bs
    out = [(0, size), (0, 1), (bs - 5, 17), (last * bs, size - last * bs)]
    return [(o, n) for o, n in out if n > 0 and o + n <= size]


def poisoned(gpu, case, par_rows, erased):
    """(objs arena, parity arena) with every erased block overwritten with
    POISON: data blocks up to `size`, coding blocks whole."""
    k, bs, size, n, g = case.k, case.bs, case.size, case.n, case.guard
    snap, _ = case.dev(gpu)
    work, par = snap.clone(), U.parity_arena(gpu, case, par_rows)
    for e in erased:
        if e < k:
            lo, hi = e * bs, min((e + 1) * bs, size)
            if lo < hi:
                work[g:g + n, lo:hi] = H.POISON
        else:
            par[1:1 + n, (e - k) * bs:(e - k + 1) * bs] = H.POISON
    return work, par


def out_width(off, length):
    return (off % 16 + length + 15) // 16 * 16 + 32


def out_arena(gpu, case, off, length):
    return case.arena(gpu, out_width(off, length), OUT_FILL)


def expected_out(gpu, case, rows, off, length):
    """The out arena after the call: `rows`' bytes of the range at [lead,
    lead + length) of every object's row, the fill everywhere else."""
    lead = off % 16
    want = np.full((case.n, out_width(off, length)), OUT_FILL, dtype=np.uint8)
    want[:, lead:lead + length] = rows[:, off:off + length]
    return case.arena(gpu, want, OUT_FILL)


def run_read(gpu, le, case, erased, off, length, what, knob=""):
    """One device.read of the range over fresh arenas, from consistent parity;
    returns the errors."""
    g, n = case.guard, case.n
    work, par = poisoned(gpu, case, case.parity, erased)
    work_snap, par_snap = work.clone(), par.clone()
    out = out_arena(gpu, case, off, length)
    ret = le.device.read(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], list(erased), off,
                         length, out=out[1:1 + n])
    gpu.cuda.synchronize()
    assert ret.data_ptr() == out[1:1 + n].data_ptr()
    ctx = f"read {knob}{case.ident()} bs {case.bs} [{off}, {off + length}) erased {what} {list(erased)}"
    return [e for e in (H.arena_diff(gpu, out, expected_out(gpu, case, case.rows, off, length), 1, f"{ctx}: out"),
                        H.arena_diff(gpu, work, work_snap, g, f"{ctx}: objs"),
                        H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity")) if e]
