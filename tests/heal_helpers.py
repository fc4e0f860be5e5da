"""Shared pieces of the heal tests (test_heal_cpu.py, no GPU;
test_device_heal.py, product library; test_heal_forms.py, the measurement
build's generic form): the per-object masks of the edge harness
(gpu_helpers.EdgeCase), one leoec_heal_dev call over poisoned arenas with
every byte compared afterwards, and the field arithmetic that applies
leoec_heal_rows' coefficient rows to blocks on the host."""
import itertools

import numpy as np

import gpu_helpers as H
import restate_np

# the edge families plus the two GF(2^8) shapes outside one gf8_heal launch
FAMILIES = H.EDGE_FAMILIES + [("vandrs", 20, 4, 8, 8704), ("vandrs", 6, 5, 8, 8704)]
GF8_FAMILIES = H.EDGE_FAMILIES[:4]  # the fused configurations at 256 lanes
EDGE_N = 9                          # objects per batch: one per mask of edge_masks

PREFILL = 0x7EA1F00D                # every unhealed word before the call
SENTINELS = (0x5EED0001, 0x5EED0002)  # the words before and after the covered ones


def family_id(f):
    return "%s-%d-%d-%d-B%d" % f


def fused(cls, k, m, w):
    """The configurations the header promises one launch for."""
    return cls in ("vandrs", "isars") and w == 8 and k <= 16 and m <= 4


def bits(ids):
    return sum(1 << b for b in set(ids))


def ids_of(mask):
    return [b for b in range(32) if (mask >> b) & 1]


def edge_masks(k, m):
    """The per-object masks of an EDGE_N-object batch (pure): clean; the last
    m data blocks (ragged and empty outputs, every survivor full); {0, k-1}
    plus coding blocks up to m; {k-1} alone; the first m data blocks; all m
    coding blocks; the last coding block alone; m + 1 blocks and a bit at
    k + m (both unrecoverable)."""
    return [0,
            bits(range(k - m, k)),
            bits(([0, k - 1] + list(range(k, k + m)))[:m]),
            bits([k - 1]),
            bits(range(m)),
            bits(range(k, k + m)),
            bits([k + m - 1]),
            bits(range(k - 1, k + m)),
            bits([0, k + m])]


RUN_N = 12  # objects per batch of run_masks


def run_masks(k, m):
    """The per-object masks of a RUN_N-object batch with runs of equal masks
    (pure), what a scrub after a lost disk hands to heal: a = {k-1} three
    times, two clean objects, b = {0, k-1} plus coding blocks up to m twice,
    U = m + 1 blocks (unrecoverable) twice, c = all m coding blocks once, a
    twice.  A run at the front and one at the back, a clean and an
    unrecoverable run, every run abutting the next; with nobj = RUN_N - 1 the
    last run is cut."""
    a = bits([k - 1])
    b = bits(([0, k - 1] + list(range(k, k + m)))[:m])
    c = bits(range(k, k + m))
    U = bits(range(k - 1, k + m))
    return [a, a, a, 0, 0, b, b, U, U, c, a, a]


def runs_of(masks):
    """[(mask, first object, objects)] of the runs of consecutive equal masks."""
    out = []
    for o, mask in enumerate(masks):
        if out and out[-1][0] == mask:
            out[-1][2] += 1
        else:
            out.append([mask, o, 1])
    return [tuple(r) for r in out]


def recoverable(mask, k, m):
    return bin(mask).count("1") <= m and mask >> (k + m) == 0


def all_masks(k, m, lo=0, hi=None):
    """Every mask with lo..hi (default m) bits set among k + m, by bit count."""
    hi = m if hi is None else hi
    return [bits(c) for p in range(lo, hi + 1) for c in itertools.combinations(range(k + m), p)]


def unrecoverable_masks(k, m, n=8):
    """n masks a (k, m) code cannot heal: alternately m + 1 bits and a high bit."""
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append(bits((i + j) % (k + m) for j in range(m + 1)))
        else:
            out.append(bits([i % k, k + m + (i % (32 - k - m))]))
    return out


def run_heal(gpu, le, case, masks, nobj=None):
    """One device.heal over clones of the case's arenas with the lost blocks
    of object o (masks[o]) poisoned, data blocks only up to `size`; unhealed
    in a pre-filled [n + 2] tensor of which the call covers words 1..n.
    Returns the list of errors: objects [0, nobj) that can be healed must be
    back to the snapshots byte for byte, everything else (the unrecoverable
    objects, the objects past nobj, guard rows, bytes past `size`) as it was
    poisoned; unhealed == 0 / mask between intact sentinels, PREFILL past
    nobj; lost unchanged."""
    k, m, bs, size, n, g = case.k, case.m, case.bs, case.size, case.n, case.guard
    nobj = n if nobj is None else nobj
    assert len(masks) == n
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    want, par_want = snap.clone(), par_snap.clone()
    for o, mask in enumerate(masks):
        healed = o < nobj and recoverable(mask, k, m)
        for b in ids_of(mask):
            if b < k:
                lo, hi = b * bs, min((b + 1) * bs, size)
                if lo < hi:
                    work[g + o, lo:hi] = H.POISON
                    if not healed:
                        want[g + o, lo:hi] = H.POISON
            elif b < k + m:
                lo = (b - k) * bs
                par[1 + o, lo:lo + bs] = H.POISON
                if not healed:
                    par_want[1 + o, lo:lo + bs] = H.POISON
    lost_host = np.array(masks, dtype=np.uint32).view(np.int32)
    lost = gpu.from_numpy(lost_host.copy()).cuda()
    unhealed = gpu.full((n + 2,), PREFILL, dtype=gpu.int32, device="cuda")
    unhealed[0], unhealed[n + 1] = SENTINELS
    out = le.device.heal(case.cls, case.params, work[g:g + n], size, par[1:1 + n], lost, nobj=nobj,
                         unhealed=unhealed[1:1 + n])
    gpu.cuda.synchronize()
    assert out.data_ptr() == unhealed[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in unhealed.cpu().tolist()]
    expect = [SENTINELS[0]] + [0 if recoverable(mk, k, m) else mk for mk in masks[:nobj]] + \
        [PREFILL] * (n - nobj) + [SENTINELS[1]]
    ctx = f"heal {case.ident()} bs {bs} nobj {nobj}"
    errors = []
    if got != expect:
        bad = [i - 1 for i in range(n + 2) if got[i] != expect[i]]
        errors.append(f"{ctx}: unhealed differs at words {bad[:8]} (-1 / {n}: sentinels): got "
                      f"{[hex(got[i + 1]) for i in bad[:8]]}, expected "
                      f"{[hex(expect[i + 1]) for i in bad[:8]]}, masks "
                      f"{[hex(masks[i]) if 0 <= i < n else None for i in bad[:8]]}")
    if not np.array_equal(lost.cpu().numpy(), lost_host):
        errors.append(f"{ctx}: lost was written")
    for err in (H.arena_diff(gpu, work, want, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par_want, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    return errors


# ---------------------------------------------------------------------------
# leoec_heal_rows' coefficient rows applied to blocks on the host.

_mulx = {}


def _shifts(oracle, w, c):
    """c * 2^x in GF(2^w) for x < w: multiplication by c is linear over GF(2).
    w <= 16: the numpy restatement's field (tests/restate_np.py, the suite's
    cross-check of the oracle); w = 32: the oracle's product (the restatement
    has no log tables that large)."""
    key = (w, c)
    if key not in _mulx:
        if w in restate_np.POLY:
            F = _mulx.setdefault(("F", w), restate_np.GF(w))
            _mulx[key] = [F.mul(c, 1 << x) for x in range(w)]
        else:
            _mulx[key] = [oracle.gf_mul(c, 1 << x, w) for x in range(w)]
    return _mulx[key]


def bitsliced(cls):
    """cauchyrs and liberation blocks are w packets, packet x holding bit x of
    every symbol; vandrs and isars blocks are little-endian w-bit words."""
    return cls in ("cauchyrs", "liberation")


def _words_scale(sh, sym):
    out = np.zeros_like(sym)
    for x, cx in enumerate(sh):
        out ^= ((sym >> x) & 1) * np.array(cx, dtype=sym.dtype)
    return out


def gf_scale(oracle, cls, w, c, block):
    """c * block, symbol by symbol, as a uint8 array of the block's length."""
    sh = _shifts(oracle, w, c)
    if bitsliced(cls):
        pk = block.reshape(w, -1)
        out = np.zeros_like(pk)
        for x in range(w):
            for l in range(w):
                if (sh[x] >> l) & 1:
                    out[l] ^= pk[x]
        return out.reshape(-1)
    if w == 8:  # the product of every byte value, once per c
        if ("lut", c) not in _mulx:
            _mulx[("lut", c)] = _words_scale(sh, np.arange(256, dtype=np.uint8))
        return _mulx[("lut", c)][block]
    dt = {16: np.dtype("<u2"), 32: np.dtype("<u4")}[w]
    return _words_scale(sh, block.view(dt)).view(np.uint8)


def apply_rows(oracle, cls, w, rows, survivors):
    """[XOR_j rows[r][j] * survivors[j]] for every row."""
    outs = []
    for row in rows:
        acc = np.zeros_like(survivors[0])
        for c, blk in zip(row, survivors):
            if c:
                acc ^= gf_scale(oracle, cls, w, c, blk)
        outs.append(acc)
    return outs
