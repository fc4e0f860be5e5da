"""Shared helpers of the GPU parity tests (test_gpu_parity.py, product
library) and the measurement-form tests (test_measure_forms.py, their own
process with LEOEC_LIBRARY=measure)."""
import ctypes

import numpy as np


def rand_bytes(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, n, dtype=np.uint8).tobytes()


def batch(gpu, n, size, stride, seed):
    """n random rows of `stride` bytes, host copy and device copy."""
    rng = np.random.Generator(np.random.PCG64(seed))
    host = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    return host, gpu.from_numpy(host).cuda()


def capi_case(le, oracle, cls, k, m, w, size, seed):
    """Inputs and oracle answers for one object, as numpy buffers for the C ABI."""
    data = np.frombuffer(rand_bytes(size, seed), dtype=np.uint8).copy()
    ref = oracle.encode(cls, k, m, w, data.tobytes())
    bs, filled = le.layout(cls, (k, m, w), size)
    return {"cls": cls, "cid": le._lib.CODING_IDS[cls], "p": (k, m, w), "size": size, "bs": bs,
            "filled": filled, "data": data, "ref": ref,
            "blocks": [np.frombuffer(b, dtype=np.uint8).copy() for b in ref]}


def capi_ops(le, c, t):
    """encode, decode (m blocks lost) and repair (2 blocks) of one case
    through the C ABI, each independent of the others' outcome (decode and
    repair read the oracle's blocks).  Returns {op: (rc, equal, detail)}."""
    L = le.lib
    k, m, w = c["p"]
    bs, filled, size = c["bs"], c["filled"], c["size"]
    res = {}
    out = np.empty(max((k + m - filled) * bs, 1), dtype=np.uint8)
    rc = L.leoec_encode(c["cid"], k, m, w, c["data"].ctypes.data, size, out.ctypes.data, out.size)
    res["encode"] = (rc, b"".join(c["ref"][filled:]) == out[:(k + m - filled) * bs].tobytes(),
                     f"{c['cls']}{c['p']} size {size}")
    lost = sorted({(t * 7 + j * 3) % (k + m) for j in range(m)})
    ids = [b for b in range(k + m) if b not in lost][::-1]
    ptrs = (ctypes.c_void_p * len(ids))(*[c["blocks"][b].ctypes.data for b in ids])
    idv = (ctypes.c_int * len(ids))(*ids)
    dec = np.empty(max(size, 1), dtype=np.uint8)
    rc = L.leoec_decode(c["cid"], k, m, w, ptrs, idv, len(ids), bs, size, dec.ctypes.data)
    res["decode"] = (rc, bool(np.array_equal(dec[:size], c["data"])),
                     f"{c['cls']}{c['p']} lost {lost}")
    res["decode_lost_data"] = any(b < k for b in lost)
    rep = sorted({t % (k + m), (t + 5) % (k + m)})
    avail = [b for b in range(k + m) if b not in rep]
    ptrs = (ctypes.c_void_p * len(avail))(*[c["blocks"][b].ctypes.data for b in avail])
    idv = (ctypes.c_int * len(avail))(*avail)
    repv = (ctypes.c_int * len(rep))(*rep)
    ro = np.empty(len(rep) * bs, dtype=np.uint8)
    rc = L.leoec_repair(c["cid"], k, m, w, ptrs, idv, len(avail), bs, repv, len(rep),
                        ro.ctypes.data)
    res["repair"] = (rc, ro.tobytes() == b"".join(c["ref"][b] for b in rep),
                     f"{c['cls']}{c['p']} {rep}")
    return res


def capi_roundtrip(le, c, t):
    """capi_ops; returns the first failing op as an error string, or None."""
    res = capi_ops(le, c, t)
    for op in ("encode", "decode", "repair"):
        rc, eq, detail = res[op]
        if rc or not eq:
            return f"{op} {detail} rc {rc}"
    return None


MIXED_SPECS = [("vandrs", 10, 4, 8, 1048576), ("vandrs", 10, 4, 8, 1048576),
               ("vandrs", 10, 4, 8, 300001), ("cauchyrs", 10, 4, 8, 1048576 + 77),
               ("isars", 10, 4, 8, 65536 + 7), ("liberation", 4, 2, 7, 777777),
               ("vandrs", 4, 2, 16, 123457), ("vandrs", 6, 3, 32, 99999),
               ("vandrs", 10, 4, 8, 9 << 20), ("cauchyrs", 4, 2, 3, 5000),
               ("vandrs", 20, 6, 8, 2000003)]


def mixed_callers(le, oracle, fail_bs=None, threads=24, rounds=8):
    """Cross-call batching (hostq.cpp): `threads` threads call the C ABI at
    once with mixed classes, widths, sizes (ragged, and 9 MiB objects above
    the batch cap, which take the per-thread path) and erasure patterns, so
    one batch holds several different maps (several launches) and identical
    maps are merged into one launch.  Every result must equal the oracle's.
    fail_bs (measurement build, LEOEC_HOSTQ_FAIL_BS): the batched launches of
    that block size report a HIP error; exactly those calls must fail with
    LEOEC_E_HIP — the encode, the repair, and the decode when it has a data
    block to rebuild — while every other call in the same batches succeeds.
    Returns the list of errors (empty: pass) and the number of injected
    failures seen."""
    import concurrent.futures as cf
    cases = [capi_case(le, oracle, *sp, seed=100 + i) for i, sp in enumerate(MIXED_SPECS)]
    E_HIP = le._lib.E_HIP

    def worker(t):
        failed = 0
        for r in range(rounds):
            c = cases[(t + r) % len(cases)]
            res = capi_ops(le, c, t + r)
            for op in ("encode", "decode", "repair"):
                rc, eq, detail = res[op]
                inject = fail_bs is not None and c["bs"] == fail_bs and (
                    op != "decode" or res["decode_lost_data"])
                if inject:
                    if rc != E_HIP:
                        return f"thread {t}: {op} {detail}: expected the injected failure, rc {rc}", 0
                    failed += 1
                elif rc or not eq:
                    return f"thread {t}: {op} {detail} rc {rc}", 0
        return None, failed

    with cf.ThreadPoolExecutor(threads) as ex:
        res = list(ex.map(worker, range(threads)))
    return [e for e, _ in res if e], sum(f for _, f in res)


# ---------------------------------------------------------------------------
# Device-batch edge harness (test_device_edges.py, test_measure_forms.py):
# one device call inside guarded arenas, every byte of every arena checked.
#
# include/leoec.h promises that bytes past `size` in an object row are read as
# zero and never touched, and that decode rebuilds erased data blocks clipped
# to `size`.  Every kernel family decides wave-uniformly between a full tile
# (unguarded 16-byte stores) and an edge tile from a minimum over its shards'
# valid lengths; these cases put a ragged or empty block on the output side
# of that decision, with non-zero bytes behind every row.

# (class, k, m, w, B): B is the target block size of the family's large
# sizes: 2 1/8 tiles of the family's widest shipped tile, so every block (or
# packet, B / w bytes) has whole tiles and a last partial one.
#   gf8_apply: 4,096 B of the block per tile (256 lanes)       -> B = 8,704
#   gfs_apply: 4,096 B of the block per tile                   -> B = 8,704
#   gfbit_apply: 2,048 B of a packet (w <= 11: 8-byte lanes)   -> B = 4,352 w
#   lib / libb / libb_dec: 1,024 B of a packet (64 lanes)      -> B = 2,176 w
#   bit_apply (cauchyrs, w > 16): 4,096 B of a packet          -> B = 8,704 w
# The last vandrs row is gf8_apply's 64-lane form (blocks above 160 KiB,
# 1 KiB tiles).
EDGE_FAMILIES = [
    ("vandrs", 10, 4, 8, 8704), ("vandrs", 4, 2, 8, 8704), ("isars", 10, 4, 8, 8704),
    ("vandrs", 7, 3, 8, 8704),
    ("cauchyrs", 10, 4, 8, 4352 * 8), ("cauchyrs", 6, 3, 4, 4352 * 4),
    ("cauchyrs", 5, 2, 11, 4352 * 11),
    ("liberation", 4, 2, 7, 2176 * 7), ("liberation", 10, 2, 11, 2176 * 11),
    ("vandrs", 10, 4, 16, 8704), ("vandrs", 6, 3, 32, 8704),
    ("vandrs", 10, 4, 8, 164992),
    ("cauchyrs", 5, 3, 17, 8704 * 17),
]
EDGE_N = 5  # objects per batch: the oracle encodes every one


def edge_sizes(k, w, B):
    """Object sizes around the block geometry (pure: no GPU, no torch).  The
    layout is bs = round_up(ceil(size / (k w)), 16) w, so for a block size B
    the last block's valid length v = size - (k - 1) bs lies in
    (B - 16 k w, B]: size = k B - d spans that range (whole, one byte short,
    either side of a 16-byte lane, past a packet's first lane, the shortest
    last block this B allows).  Then the small objects whose trailing data
    blocks are empty: v = 0, v = 5, the last block empty and the one before
    it ragged, and one byte."""
    assert B % (16 * w) == 0 and B >= 16 * w
    big = [k * B - d for d in (0, 1, 15, 16, 17, 16 * w + 5, 16 * k * w - 1)]
    small = [16 * w * (k - 1), 16 * w * (k - 1) + 5, 16 * w * (k - 2) + 5, 1]
    out = []
    for s in big + small:
        if s > 0 and s not in out:
            out.append(s)
    return out


def block_valids(k, bs, size):
    """Valid bytes of each data block of an object of `size` bytes."""
    return [min(max(size - j * bs, 0), bs) for j in range(k)]


def gfbk_straddles(bs, v, tile):
    """gfbk_apply (w = 8, `tile` bytes of every packet per workgroup): a tile
    that lies inside the packet (t0 + tile <= ps) reaches past a last block of
    v valid bytes in packet 7."""
    ps = bs // 8
    return ps >= tile and 0 < v and ps % tile < bs - v


# cauchyrs(10,4,8), bs 66,560 (packets of 8,320 B), v 65,281: gfbk_straddles
# at the 1,024-, 2,048- and 4,096-byte tiles of gfbk_apply's 64-, 128- and
# 256-lane forms (8,320 = 2 x 4,096 + 128)
GFBK_WIDE_SIZE = 10 * 66560 - 1279


def edge_erasures(k, m):
    """Decode erasure sets: the last m data blocks (ragged and empty outputs,
    every survivor full); the first and last data block plus coding blocks
    (a ragged output, data and coding survivors); the last block alone; the
    first m (the ragged block a survivor); the last two."""
    sets = [list(range(k - m, k)), ([0, k - 1] + list(range(k, k + m)))[:m], [k - 1],
            list(range(m))]
    if m >= 2:
        sets.append([k - 2, k - 1])
    out = []
    for s in sets:
        s = sorted(set(s))
        if s not in out:
            out.append(s)
    return out


def edge_repairs(k, m):
    out = []
    for s in ([k - 1, k], [0, k // 2, k, k + m - 1][:m]):
        s = sorted(set(s))
        if s not in out:
            out.append(s)
    return out


GUARD_FILL, PARITY_FILL, REPAIR_FILL, POISON = 0xC3, 0x5A, 0x3C, 0xA5


class EdgeCase:
    """n objects of one (class, k, m, w, size): host bytes (random data,
    random non-zero bytes from `size` to the row stride), the oracle's blocks
    of every object, and (lazily) the device arenas' snapshots."""

    def __init__(self, le, oracle, cfg, size, n):
        self.cls, self.k, self.m, self.w = cfg
        self.params = cfg[1:]
        self.size, self.n = size, n
        k, m, w = self.params
        self.bs, _ = le.layout(self.cls, self.params, size)
        bs = self.bs
        # rows 16-byte aligned at every 16-byte phase; the next row starts
        # 32-47 bytes past the object
        self.stride = (size + 15) // 16 * 16 + 32
        # guard rows before and after: at least one whole row each, and
        # enough that a whole-block (k bs) overrun of the last row stays
        # inside the allocation (tiny objects: k bs is many rows)
        self.guard = max(1, -(-k * bs // self.stride))
        seed = size * 31 + k * 7 + m * 3 + w
        self.rows = np.empty((n, self.stride), dtype=np.uint8)
        self.rows[:, :size] = np.frombuffer(rand_bytes(n * size, seed), dtype=np.uint8).reshape(n, size)
        rng = np.random.Generator(np.random.PCG64(seed + 1))
        self.rows[:, size:] = rng.integers(1, 256, (n, self.stride - size), dtype=np.uint8)
        self.blocks = np.empty((k + m, n, bs), dtype=np.uint8)
        for o in range(n):
            ref = oracle.encode(self.cls, k, m, w, self.rows[o, :size].tobytes())
            for b in range(k + m):
                self.blocks[b, o] = np.frombuffer(ref[b], dtype=np.uint8)
        self.parity = np.concatenate([self.blocks[k + i] for i in range(m)], axis=1)
        self.slack = rng.integers(1, 256, (k + m, n, 32), dtype=np.uint8)  # behind repair's blocks
        self._dev = None

    def ident(self):
        return (self.cls,) + tuple(self.params) + (self.size,)

    def arena(self, gpu, rows, fill, guard=1):
        """[guard + n + guard, stride] device tensor: `fill` in the guard
        rows, `rows` (or `fill` where rows is an int width) between them."""
        n = self.n
        if isinstance(rows, int):
            return gpu.full((n + 2 * guard, rows), fill, dtype=gpu.uint8, device="cuda")
        host = np.full((n + 2 * guard, rows.shape[1]), fill, dtype=np.uint8)
        host[guard:guard + n] = rows
        return gpu.from_numpy(host).cuda()

    def dev(self, gpu):
        """Snapshots (never written): the objs arena and the parity arena
        holding the oracle's coding blocks, parity_stride = m bs + 48."""
        if self._dev is None:
            par = np.full((self.n, self.m * self.bs + 48), GUARD_FILL, dtype=np.uint8)
            par[:, :self.m * self.bs] = self.parity
            self._dev = (self.arena(gpu, self.rows, GUARD_FILL, self.guard),
                         self.arena(gpu, par, GUARD_FILL))
        return self._dev


_edge_cases = {}


def edge_case(le, oracle, cfg, size, n=EDGE_N):
    """The EdgeCase of (cfg, size), computed once and shared (the cases of
    one configuration at a time are kept)."""
    if _edge_cases and next(iter(_edge_cases))[0] != cfg:
        _edge_cases.clear()
    key = (cfg, size, n)
    if key not in _edge_cases:
        _edge_cases[key] = EdgeCase(le, oracle, cfg, size, n)
    return _edge_cases[key]


def arena_diff(gpu, got, want, guard, what):
    """None when every byte of the arena `got` equals `want`; otherwise where
    they differ (rows counted from the first object's; negative and >= n are
    guard rows)."""
    if gpu.equal(got, want):
        return None
    ne = (got != want).nonzero()
    r, c = int(ne[0, 0]), int(ne[0, 1])
    rows = sorted({int(x) - guard for x in ne[:, 0].unique().cpu()})
    return (f"{what}: {ne.shape[0]} bytes differ in rows {rows} (row stride {got.shape[1]}); first at "
            f"row {r - guard} byte {c}: got 0x{int(got[r, c]):02X}, expected 0x{int(want[r, c]):02X}")


def check_decode(gpu, le, case, erased):
    """In-place device decode of `erased` over poisoned data blocks: every
    byte of the objs arena (guard rows, every row's bytes past `size`) back
    to the original, the parity arena untouched.  Returns None or the error."""
    k, bs, size, n, g = case.k, case.bs, case.size, case.n, case.guard
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    objs = work[g:g + n]
    for e in erased:
        lo, hi = e * bs, min((e + 1) * bs, size)
        if e < k and lo < hi:
            objs[:, lo:hi] = POISON
    le.device.decode(case.cls, case.params, objs, size, par[1:1 + n], list(erased))
    gpu.cuda.synchronize()
    ctx = f"{case.ident()} bs {bs} erased {list(erased)}"
    return (arena_diff(gpu, work, snap, g, f"decode {ctx}: objs") or
            arena_diff(gpu, par, par_snap, 1, f"decode {ctx}: parity"))


def check_encode(gpu, le, case):
    """Device encode into a 0x5A-filled parity arena: the oracle's coding
    blocks in bytes [0, m bs) of every object's row, 0x5A everywhere else,
    the objs arena untouched."""
    m, bs, n, g = case.m, case.bs, case.n, case.guard
    snap, _ = case.dev(gpu)
    work = snap.clone()
    want = np.full((n, m * bs + 48), PARITY_FILL, dtype=np.uint8)
    want[:, :m * bs] = case.parity
    want = case.arena(gpu, want, PARITY_FILL)
    par = case.arena(gpu, m * bs + 48, PARITY_FILL)
    le.device.encode(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n])
    gpu.cuda.synchronize()
    ctx = f"{case.ident()} bs {bs}"
    return (arena_diff(gpu, par, want, 1, f"encode {ctx}: parity") or
            arena_diff(gpu, work, snap, g, f"encode {ctx}: objs"))


def check_repair(gpu, le, case, lost):
    """Device repair of `lost` from every other block: blocks in
    [n + 2, bs + 32] arenas with random bytes behind them, outputs in
    0x3C-filled [n + 2, bs + 48] arenas; the oracle's blocks in bytes
    [0, bs) of every object's row, 0x3C everywhere else, inputs untouched."""
    k, m, bs, n = case.k, case.m, case.bs, case.n
    snaps, avail = {}, []
    for b in range(k + m):
        if b in lost:
            avail.append(None)
            continue
        snaps[b] = case.arena(gpu, np.concatenate([case.blocks[b], case.slack[b]], axis=1), GUARD_FILL)
        avail.append(snaps[b].clone())
    outs = [case.arena(gpu, bs + 48, REPAIR_FILL) for _ in lost]
    le.device.repair(case.cls, case.params, [a if a is None else a[1:1 + n] for a in avail], bs,
                     list(lost), [o[1:1 + n] for o in outs], n)
    gpu.cuda.synchronize()
    ctx = f"{case.ident()} bs {bs} lost {list(lost)}"
    for o, b in zip(outs, lost):
        want = np.full((n, bs + 48), REPAIR_FILL, dtype=np.uint8)
        want[:, :bs] = case.blocks[b]
        err = arena_diff(gpu, o, case.arena(gpu, want, REPAIR_FILL), 1, f"repair {ctx}: block {b}")
        if err:
            return err
    for b, s in snaps.items():
        err = arena_diff(gpu, avail[b], s, 1, f"repair {ctx}: input block {b}")
        if err:
            return err
    return None
