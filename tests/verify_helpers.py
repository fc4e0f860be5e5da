"""Shared pieces of the device verify tests (test_device_verify.py, product
library; test_verify_forms.py, the measurement build's two-pass form): the
damaged batches of the edge harness (gpu_helpers.EdgeCase) and what
leoec_verify_dev must answer for them."""
import gpu_helpers as H

# the edge families plus the two GF(2^8) shapes outside one gf8_check launch
# (k > 16: accumulating encode launches; m > 4: two row groups), both two-pass
FAMILIES = H.EDGE_FAMILIES + [("vandrs", 20, 4, 8, 8704), ("vandrs", 6, 5, 8, 8704)]
GF8_FAMILIES = H.EDGE_FAMILIES[:4]  # the fused configurations at 256 lanes

BIT = 0x10            # the bit flipped in a damaged byte
PREFILL = 0xFFFFFFFF  # every flag word before the call
SENTINELS = (0x5EED0001, 0x5EED0002)  # the words before and after the covered ones


def family_id(f):
    return "%s-%d-%d-%d-B%d" % f


def fused(cls, k, m, w):
    """The configurations the header promises a workspace-free check for."""
    return cls in ("vandrs", "isars") and w == 8 and k <= 16 and m <= 4


def packet_tile(cls, w):
    """Bytes of a packet per workgroup in the bitmatrix families' encode
    kernels (gpu_helpers.EDGE_FAMILIES' table); None for the byte kernels."""
    if cls == "cauchyrs":
        return 2048 if w <= 11 else 4096
    if cls == "liberation":
        return 1024
    return None


def damage(case, second):
    """[(arena, object, byte of the object's row)] of one call.  First call:
    coding block 0 at byte 0, coding block m-1 at its last byte, the last
    valid data byte.  Second call: objects 0 and 1 at the first byte of the
    last partial tile of the block (byte kernels: 4 KiB tiles; bitmatrix
    families: of the last packet), object 2 at data byte 0."""
    m, w, bs, size = case.m, case.w, case.bs, case.size
    if not second:
        return [("parity", 0, 0), ("parity", 1, (m - 1) * bs + bs - 1), ("objs", 2, size - 1)]
    tile = packet_tile(case.cls, w)
    if tile is None:
        p = (bs - 1) // 4096 * 4096
    else:
        ps = bs // w
        p = (w - 1) * ps + (ps - 1) // tile * tile
    return [("parity", 0, p), ("parity", 1, (m - 1) * bs + p), ("objs", 2, 0)]


def data_damage_mask(oracle, case, o, pos):
    """Flag word of object o with data byte pos damaged, from the oracle:
    re-encode the damaged data, compare with the stored coding blocks."""
    k, m, w = case.params
    data = bytearray(case.rows[o, :case.size].tobytes())
    data[pos] ^= BIT
    ref = oracle.encode(case.cls, k, m, w, bytes(data))
    return sum(1 << i for i in range(m) if ref[k + i] != case.blocks[k + i, o].tobytes())


def expected_flags(oracle, case, second):
    """[1 << 0, 1 << (m-1), M, 0, 0] with M from the oracle; every code here
    is MDS, so M must name every coding block."""
    m = case.m
    dmg = damage(case, second)
    M = data_damage_mask(oracle, case, 2, dmg[2][2])
    assert M == (1 << m) - 1, (case.ident(), second, M)
    return [1 << 0, 1 << (m - 1), M] + [0] * (case.n - 3)


def run_verify(gpu, le, case, dmg, nobj=None, workspace=None):
    """One device.verify over damaged clones of the case's arenas, flags in a
    pre-filled [n + 2] tensor of which the call covers words 1..n.  Returns
    (the n covered words, error or None): the sentinels intact and every
    byte of both arenas, guard rows included, as it was before the call."""
    n, g = case.n, case.guard
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    for where, o, pos in dmg:
        row = work[g + o] if where == "objs" else par[1 + o]
        row[pos] ^= BIT
    work_snap, par_snap = work.clone(), par.clone()
    flags = gpu.full((n + 2,), -1, dtype=gpu.int32, device="cuda")
    flags[0], flags[n + 1] = SENTINELS
    out = le.device.verify(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], nobj=nobj,
                           flags=flags[1:1 + n], workspace=workspace)
    gpu.cuda.synchronize()
    assert out.data_ptr() == flags[1:1 + n].data_ptr()
    got = [int(x) & 0xFFFFFFFF for x in flags.cpu().tolist()]
    ctx = f"verify {case.ident()} bs {case.bs} damage {dmg} nobj {nobj}"
    err = None
    if (got[0], got[-1]) != SENTINELS:
        err = f"{ctx}: sentinel words {got[0]:#x}, {got[-1]:#x}"
    err = err or (H.arena_diff(gpu, work, work_snap, g, f"{ctx}: objs") or
                  H.arena_diff(gpu, par, par_snap, 1, f"{ctx}: parity"))
    return got[1:-1], err


def check_case(gpu, le, oracle, case):
    """Both damaged batches of one case; the list of errors."""
    errors = []
    for second in (False, True):
        want = expected_flags(oracle, case, second)
        got, err = run_verify(gpu, le, case, damage(case, second))
        if err:
            errors.append(err)
        if got != want:
            errors.append(f"verify {case.ident()} bs {case.bs} call {1 + second}: flags "
                          f"{[hex(x) for x in got]}, expected {[hex(x) for x in want]}")
    return errors
