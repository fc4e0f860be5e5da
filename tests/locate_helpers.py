"""Shared pieces of the locate tests (test_locate_cpu.py, no GPU;
test_device_locate.py, product library): the families, the damaged batches of
the edge harness (gpu_helpers.EdgeCase) beyond verify_helpers.damage, and a
numpy host model of what leoec_locate_dev must answer: the syndromes of
oracle-encoded blocks, tested with leoec_locate_rows' ratios through GF(2^8)
products taken from the oracle."""
import numpy as np

import gpu_helpers as H
import verify_helpers as V

# the fused configurations at 256 lanes, gf8_locate's 64-lane form (blocks
# above 160 KiB, 1 KiB tiles) and the widest instance (K = 16, R = 4)
FAMILIES = V.GF8_FAMILIES + [("vandrs", 10, 4, 8, 164992), ("vandrs", 16, 4, 8, 8704)]

MANY = 0x80000000      # LEOEC_LOCATE_MANY
BIT = V.BIT            # the bit flipped in a damaged byte
PREFILL = 0x10CA7E00   # every lost word before the call
SENTINELS = V.SENTINELS

family_id = V.family_id


def served(cls, k, m, w):
    """The configurations the header promises an answer for."""
    return cls in ("vandrs", "isars") and w == 8 and k <= 16 and 2 <= m <= 4


# ---------------------------------------------------------------------------
# Damage lists: [(arena, object, byte of the object's row, xor value)].  Every
# position lies inside valid bytes: data below `size`, parity below m bs.

def with_bit(dmg):
    """verify_helpers.damage's triples as flips of BIT."""
    return [(where, o, pos, BIT) for where, o, pos in dmg]


def last_block(case):
    """The last data block with a valid byte."""
    return (case.size - 1) // case.bs


def multi_damage(case):
    """The third call, one pattern per object:
      0  data block 0 at its first and its last valid byte        -> 1 << 0
      1  data block 0 byte 0, the last byte of coding block 1     -> MANY
      2  m >= 3: two blocks at byte offset 0: data blocks 0 and 1 where block
         1 has a byte there, else data block 0 and coding block 0 -> MANY
         m = 2: as object 1                                       -> MANY
      3  every valid byte of the last non-empty data block XORed with a
         random non-zero byte                                     -> its bit
      4  clean                                                    -> 0"""
    k, m, bs, size = case.k, case.m, case.bs, case.size
    dmg = [("objs", 0, p, BIT) for p in sorted({0, min(bs, size) - 1})]
    dmg += [("objs", 1, 0, BIT), ("parity", 1, 2 * bs - 1, BIT)]
    if m < 3:
        dmg += [("objs", 2, 0, BIT), ("parity", 2, 2 * bs - 1, BIT)]
    elif size > bs:
        dmg += [("objs", 2, 0, BIT), ("objs", 2, bs, BIT)]
    else:
        dmg += [("objs", 2, 0, BIT), ("parity", 2, 0, BIT)]
    j = last_block(case)
    rng = np.random.Generator(np.random.PCG64(size * 13 + k))
    dmg += [("objs", 3, p, int(x)) for p, x in zip(range(j * bs, size),
                                                   rng.integers(1, 256, size - j * bs))]
    return dmg


def expected_calls(case):
    """[(damage list, expected words)] of the three calls of one case."""
    k, m, bs, size, n = case.k, case.m, case.bs, case.size, case.n
    assert n == H.EDGE_N == 5
    return [
        (with_bit(V.damage(case, False)), [1 << k, 1 << (k + m - 1), 1 << last_block(case), 0, 0]),
        (with_bit(V.damage(case, True)), [1 << k, 1 << (k + m - 1), 1 << 0, 0, 0]),
        (multi_damage(case), [1 << 0, MANY, MANY, 1 << last_block(case), 0]),
    ]


# ---------------------------------------------------------------------------
# The host model.

_lut = {}


def gf8_lut(oracle, c):
    """c * x for every byte x, the products taken from the oracle."""
    if c not in _lut:
        _lut[c] = np.array([oracle.gf_mul(c, x, 8) for x in range(256)], dtype=np.uint8)
    return _lut[c]


def model_word(oracle, cfg, size, data, stored, ratio):
    """The word of one object.  data: its `size` bytes as they are now;
    stored: its m coding blocks as they are now; ratio: leoec_locate_rows'
    m - 1 lists.  Candidates are the blocks consistent with every byte
    column: coding block i when every other syndrome is zero everywhere, data
    block j when s_i == T[i][j] s_0 everywhere, i = 1..m-1."""
    cls, k, m, w = cfg
    ref = oracle.encode(cls, k, m, w, bytes(data))
    s = [np.frombuffer(ref[k + i], dtype=np.uint8) ^ stored[i] for i in range(m)]
    if not any(x.any() for x in s):
        return 0
    cand = [k + i for i in range(m) if not any(s[r].any() for r in range(m) if r != i)]
    for j in range(k):
        if all(np.array_equal(gf8_lut(oracle, ratio[i - 1][j])[s[0]], s[i]) for i in range(1, m)):
            cand.append(j)
    return 1 << cand[0] if len(cand) == 1 else MANY


def object_blocks(case, o):
    """(data bytes, [m coding blocks]) of object o, fresh copies."""
    data = case.rows[o, :case.size].copy()
    stored = [case.blocks[case.k + i, o].copy() for i in range(case.m)]
    return data, stored


def model_words(oracle, le, case, dmg):
    """The model's words of the case's n objects under a damage list."""
    cfg = (case.cls,) + tuple(case.params)
    ratio = le.device.locate_rows(case.cls, case.params)
    objs = [object_blocks(case, o) for o in range(case.n)]
    for where, o, pos, x in dmg:
        data, stored = objs[o]
        if where == "objs":
            assert 0 <= pos < case.size
            data[pos] ^= x
        else:
            assert 0 <= pos < case.m * case.bs
            stored[pos // case.bs][pos % case.bs] ^= x
    touched = {o for _, o, _, _ in dmg}
    return [model_word(oracle, cfg, case.size, *objs[o], ratio) if o in touched else 0
            for o in range(case.n)]


# ---------------------------------------------------------------------------
# One device call.

def damaged_arenas(gpu, case, dmg):
    """Clones of the case's arenas with the damage applied."""
    g = case.guard
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    for where in ("objs", "parity"):
        hits = [(o, pos, x) for wh, o, pos, x in dmg if wh == where]
        if not hits:
            continue
        t, first = (work, g) if where == "objs" else (par, 1)
        rows = gpu.tensor([first + o for o, _, _ in hits], device="cuda")
        cols = gpu.tensor([pos for _, pos, _ in hits], device="cuda")
        t[rows, cols] ^= gpu.tensor([x for _, _, x in hits], dtype=gpu.uint8, device="cuda")
    return work, par


def run_locate(gpu, le, case, work, par, nobj=None):
    """One device.locate over the given arenas, lost in a pre-filled [n + 2]
    tensor of which the call covers words 1..n.  Returns (the [n + 2] tensor,
    the n covered words, error or None): the sentinels intact and every byte
    of both arenas, guard rows included, as it was before the call."""
    n, g = case.n, case.guard
    work_snap, par_snap = work.clone(), par.clone()
    lost = gpu.full((n + 2,), PREFILL, dtype=gpu.int32, device="cuda")
    lost[0], lost[n + 1] = SENTINELS
    out = le.device.locate(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], nobj=nobj,
                           lost=lost[1:1 + n])
    gpu.cuda.synchronize()
    assert out.data_ptr() == lost[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in lost.cpu().tolist()]
    ctx = f"locate {case.ident()} bs {case.bs} nobj {nobj}"
    err = None
    if (got[0], got[-1]) != SENTINELS:
        err = f"{ctx}: sentinel words {got[0]:#x}, {got[-1]:#x}"
    err = err or (H.arena_diff(gpu, work, work_snap, g, f"{ctx}: objs") or
                  H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity"))
    return lost, got[1:-1], err
