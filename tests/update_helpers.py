"""Shared pieces of the leoec_update_dev tests (test_device_update.py,
test_update_forms.py, update_wide_child.py): the families, sizes and ranges,
the expected bytes, and one update call inside gpu_helpers' guarded arenas with
every byte of objs, parity and patch compared afterwards.

Expected bytes.  The new bytes differ from the old in every byte of the range:
new[p] = old[p] ^ (1 + r % 255) with r = p - offset (pattern()), so the delta D
(old ^ new inside the range, zero elsewhere) is the same object for all the
objects of a batch and the oracle encodes it once per range:
    objs   = the snapshot with the range patched (numpy);
    parity = parity before ^ the oracle's coding blocks of D;
    patch  = as it was (poison outside [lead, lead + length) of every row: a
             byte read from there as data changes the delta).
From consistent parity (the oracle's blocks of the EdgeCase) the result is also
held against the oracle's encoding of the new object itself, for one object per
range (every object in turn); from random parity a re-encoding implementation
fails."""
import ctypes

import numpy as np

import gpu_helpers as H

# gpu_helpers.EDGE_FAMILIES, then k > 16, m > 4 (two launches of coding rows),
# m = 15 (four, the last with three rows), k + m = 34 > 32 at w = 16, and 68
# bit-rows (two launches of bit_update's 64)
FAMILIES = H.EDGE_FAMILIES + [("vandrs", 20, 4, 8, 8704), ("vandrs", 6, 5, 8, 8704),
                              ("vandrs", 16, 15, 8, 8704), ("vandrs", 30, 4, 16, 8704),
                              ("cauchyrs", 4, 4, 17, 8704 * 17)]
N = H.EDGE_N
TILES = (1024, 4096)  # bit_update's bytes of a packet, gf_update's bytes of a segment, per workgroup
PATCH_FILL = H.POISON


def family_id(f):
    return "%s-%d-%d-%d-B%d" % f


def packet_class(cls):
    return cls in ("cauchyrs", "liberation")


def sizes(family):
    """k B - 17 (a ragged last block) and the small size whose last data block
    is empty and the one before it ragged."""
    cls, k, m, w, B = family
    big, small = k * B - 17, 16 * w * (k - 2) + 5
    assert big in H.edge_sizes(k, w, B) and small in H.edge_sizes(k, w, B)
    return [big, small]


def ranges(family, size, bs):
    """[(offset, length)] of the issue's list that fit an object of `size`
    bytes, without repeats: the large size holds every one."""
    cls, k, m, w, B = family
    ps = bs // w
    last = (size - 1) // bs  # the last data block with a byte
    out = [(0, size), (0, 1), (size - 1, size), (1, 16), (15, 17), (16, 32),
           (3, 4),            # the odd (high) byte of a w = 16 word
           (6, 7),            # byte 2 of a w = 32 word
           (bs - 5, bs + 7), (bs, 2 * bs), (last * bs, size), (bs // 2, 3 * bs + 5)]
    out += [(t - 1, t + 1) for t in TILES]
    if packet_class(cls):
        out += [(ps - 3, ps + 3), (ps, 2 * ps)]
    seen = []
    for lo, hi in out:
        if 0 <= lo < hi <= size and (lo, hi - lo) not in seen:
            seen.append((lo, hi - lo))
    return seen


def pattern(length, salt=0):
    """1 + r % 255 (salt 0); another non-zero byte per position for salt 1."""
    r = np.arange(length, dtype=np.int64)
    return (1 + (r * (1 + 6 * salt) + 3 * salt) % 255).astype(np.uint8)


_deltas = {}


def delta_parity(oracle, case, offset, length, salt=0):
    """[m bs] bytes: the oracle's coding blocks of D."""
    key = (case.ident(), offset, length, salt)
    if key not in _deltas:
        if len(_deltas) > 64:
            _deltas.clear()
        k, m, w = case.params
        d = np.zeros(case.size, dtype=np.uint8)
        d[offset:offset + length] = pattern(length, salt)
        ref = oracle.encode(case.cls, k, m, w, d.tobytes())
        _deltas[key] = np.frombuffer(b"".join(ref[k:]), dtype=np.uint8).copy()
    return _deltas[key]


def random_parity(case):
    rng = np.random.Generator(np.random.PCG64(case.size * 13 + case.k))
    return rng.integers(0, 256, (case.n, case.m * case.bs), dtype=np.uint8)


def parity_arena(gpu, case, rows):
    """gpu_helpers' parity arena (stride m bs + 48, guard fill) around `rows`."""
    par = np.full((case.n, case.m * case.bs + 48), H.GUARD_FILL, dtype=np.uint8)
    par[:, :case.m * case.bs] = rows
    return case.arena(gpu, par, H.GUARD_FILL)


def patch_rows(case, offset, length, salt=0):
    """The patch rows on the host: poison, the new bytes at [lead, lead + length)."""
    lead = offset % 16
    stride = (lead + length + 15) // 16 * 16 + 32
    rows = np.full((case.n, stride), PATCH_FILL, dtype=np.uint8)
    rows[:, lead:lead + length] = case.rows[:, offset:offset + length] ^ pattern(length, salt)
    return rows


def expected(gpu, oracle, case, par_before, offset, length, salt=0):
    """(objs arena, parity arena) after the update, from the host's bytes."""
    g, n, mbs = case.guard, case.n, case.m * case.bs
    rows = case.rows.copy()
    rows[:, offset:offset + length] ^= pattern(length, salt)
    par = par_before ^ delta_parity(oracle, case, offset, length, salt)[None, :]
    return case.arena(gpu, rows, H.GUARD_FILL, g), parity_arena(gpu, case, par), rows, par


def run_update(gpu, le, oracle, case, par_before, offset, length, what, knob=""):
    """One device.update of the range over fresh arenas; returns the errors."""
    g, n = case.guard, case.n
    snap, _ = case.dev(gpu)
    work = snap.clone()
    par = parity_arena(gpu, case, par_before)
    patch_snap = case.arena(gpu, patch_rows(case, offset, length), PATCH_FILL)
    patch = patch_snap.clone()
    want, par_want, _, _ = expected(gpu, oracle, case, par_before, offset, length)
    le.device.update(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], patch[1:1 + n],
                     offset, length)
    gpu.cuda.synchronize()
    ctx = f"update {knob}{case.ident()} bs {case.bs} [{offset}, {offset + length}) from {what} parity"
    return [e for e in (H.arena_diff(gpu, work, want, g, f"{ctx}: objs"),
                        H.arena_diff(gpu, par, par_want, 1, f"{ctx}: parity"),
                        H.arena_diff(gpu, patch, patch_snap, 1, f"{ctx}: patch")) if e]


def oracle_parity_of_new(oracle, case, o, offset, length):
    """The oracle's coding blocks of object o with the range patched."""
    k, m, w = case.params
    row = case.rows[o, :case.size].copy()
    row[offset:offset + length] ^= pattern(length)
    return np.frombuffer(b"".join(oracle.encode(case.cls, k, m, w, row.tobytes())[k:]), dtype=np.uint8)


def encode_dev_of_delta(gpu, le, case, offset, length):
    """leoec_encode_dev's coding blocks of D, into a fresh buffer."""
    d = np.zeros((1, (case.size + 15) // 16 * 16), dtype=np.uint8)
    d[0, offset:offset + length] = pattern(length)
    out = gpu.zeros((1, case.m * case.bs), dtype=gpu.uint8, device="cuda")
    le.device.encode(case.cls, case.params, gpu.from_numpy(d).cuda(), case.size, out)
    gpu.cuda.synchronize()
    return out.cpu().numpy()[0]


def coding_bits(le, cls, k, m, w):
    """The (m w) x (k w) coding bitmatrix of a packet class (leoec_coding_matrix)."""
    n = m * w * k * w
    out = (ctypes.c_uint32 * n)()
    got = ctypes.c_int(0)
    rc = le._lib.lib.leoec_coding_matrix(le._lib.CODING_IDS[cls], k, m, w, out, n, ctypes.byref(got))
    assert rc == 0 and got.value == n, (rc, got.value)
    return np.array(out[:n], dtype=np.uint8).reshape(m * w, k * w)
