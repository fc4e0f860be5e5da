"""Shared pieces of the leoec_heal_ws_dev tests (test_heal_ws_cpu.py, no GPU;
test_device_heal_ws.py, test_heal_ws_forms.py and the child processes on the
device): heal_helpers.run_heal's standard for device.heal_ws (poisoned arenas
with guard rows, every byte of every buffer compared, unhealed between
sentinels, lost unchanged) plus the totals, the workspace's tail and, byte for
byte, a device.heal run over clones of the same damaged arenas."""
import numpy as np

import gpu_helpers as H
import heal_helpers as HH

TOTALS_PREFILL = 0x70771E55
WS_FILL, WS_TAIL = 0xE7, 64
TILE_GFW, TILE_BIT = 4096, 1024  # bytes of a block / of a packet per item (gfw_heal_tile.hpp, bit_heal_tile.hpp)

# the configurations the call must serve beside heal_helpers.FAMILIES, and one
# it must refuse
SERVED = [("vandrs", 20, 4, 8), ("vandrs", 6, 5, 8), ("vandrs", 10, 4, 16), ("vandrs", 6, 3, 32),
          ("cauchyrs", 10, 4, 8), ("cauchyrs", 5, 3, 17), ("liberation", 10, 2, 11),
          ("vandrs", 30, 2, 16), ("cauchyrs", 30, 2, 5)]
REFUSED = [("vandrs", 16, 15, 8)]


def sizes(family):
    """scrub_dev_helpers.sizes_and_whole: k B - 1, 16 w (k - 2) + 5 and k B."""
    cls, k, m, w, B = family
    return [k * B - 1, 16 * w * (k - 2) + 5, k * B]


def head(nobj):
    """The workspace: the header and the index words."""
    return 16 + (4 * nobj + 15) // 16 * 16


def image_bytes(cls, k, m, w):
    """The header's rule, restated: bytes of the pattern table of a code
    outside leoec_heal_dev's fused family."""
    from math import comb
    records = sum(comb(k + m, p) for p in range(1, m + 1))
    per = w if cls in ("cauchyrs", "liberation") else 1
    return 4 * (1104 + records * (8 + m * k * per))


def served(cls, k, m, w):
    return k + m <= 32 and (HH.fused(cls, k, m, w) or image_bytes(cls, k, m, w) <= 8 << 20)


def damaged(gpu, case, masks, nobj=None):
    """run_heal's arenas: (work, par) with the lost blocks of every object
    poisoned (data blocks up to `size`), (want, par_want) what a heal of
    objects [0, nobj) must leave."""
    k, m, bs, size, n, g = case.k, case.m, case.bs, case.size, case.n, case.guard
    nobj = n if nobj is None else nobj
    assert len(masks) == n
    snap, par_snap = case.dev(gpu)
    work, par = snap.clone(), par_snap.clone()
    want, par_want = snap.clone(), par_snap.clone()
    for o, mask in enumerate(masks):
        healed = o < nobj and HH.recoverable(mask, k, m)
        for b in HH.ids_of(mask):
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
    return work, par, want, par_want


def u32(t):
    return [int(x) & 0xFFFFFFFF for x in t.cpu().tolist()]


class Buffers:
    """The call's own buffers for an n-object batch: lost, unhealed in a
    pre-filled [n + 2] tensor (words 1..n covered), totals in a [4] tensor
    (words 1..2), the workspace in WS_FILL bytes with WS_TAIL more behind."""

    def __init__(self, gpu, masks):
        n = len(masks)
        self.n = n
        self.lost_host = np.array(masks, dtype=np.uint32).view(np.int32)
        self.lost = gpu.from_numpy(self.lost_host.copy()).cuda()
        self.unhealed = gpu.full((n + 2,), HH.PREFILL, dtype=gpu.int32, device="cuda")
        self.unhealed[0], self.unhealed[n + 1] = HH.SENTINELS
        self.totals = gpu.full((4,), TOTALS_PREFILL, dtype=gpu.int32, device="cuda")
        self.totals[0], self.totals[3] = HH.SENTINELS
        self.need = head(n)
        self.ws = gpu.full((self.need + WS_TAIL,), WS_FILL, dtype=gpu.uint8, device="cuda")

    def reset(self, gpu):
        n = self.n
        self.unhealed[1:1 + n] = HH.PREFILL
        self.totals[1:3] = TOTALS_PREFILL


def call(le, case, work, par, buf, nobj=None, stream=None):
    n, g = case.n, case.guard
    return le.device.heal_ws(case.cls, case.params, work[g:g + n], case.size, par[1:1 + n], buf.lost,
                             nobj=nobj, unhealed=buf.unhealed[1:1 + n], totals=buf.totals[1:3],
                             workspace=buf.ws[:buf.need], stream=stream)


def check_words(gpu, case, masks, buf, nobj, ctx):
    """unhealed, totals, lost and the workspace's tail after a call over
    objects [0, nobj)."""
    k, m, n = case.k, case.m, case.n
    errors = []
    got = u32(buf.unhealed)
    expect = [HH.SENTINELS[0]] + [0 if HH.recoverable(mk, k, m) else mk for mk in masks[:nobj]] + \
        [HH.PREFILL] * (n - nobj) + [HH.SENTINELS[1]]
    if got != expect:
        bad = [i - 1 for i in range(n + 2) if got[i] != expect[i]]
        errors.append(f"{ctx}: unhealed differs at words {bad[:8]} (-1 / {n}: sentinels): got "
                      f"{[hex(got[i + 1]) for i in bad[:8]]}, expected "
                      f"{[hex(expect[i + 1]) for i in bad[:8]]}")
    tot = u32(buf.totals)
    want_tot = [HH.SENTINELS[0],
                sum(1 for mk in masks[:nobj] if mk and HH.recoverable(mk, k, m)),
                sum(1 for mk in masks[:nobj] if not HH.recoverable(mk, k, m)), HH.SENTINELS[1]]
    if tot != want_tot:
        errors.append(f"{ctx}: totals {tot[1:3]} between {[hex(tot[0]), hex(tot[3])]}, expected "
                      f"{want_tot[1:3]} between the sentinels")
    if not np.array_equal(buf.lost.cpu().numpy(), buf.lost_host):
        errors.append(f"{ctx}: lost was written")
    if not bool((buf.ws[buf.need:] == WS_FILL).all()):
        errors.append(f"{ctx}: workspace written past its {buf.need} bytes")
    return errors


def run_heal_ws(gpu, le, case, masks, nobj=None, reference=True, invoke=None):
    """One device.heal_ws over the damaged arenas of `masks` (invoke(work,
    par, buf): another way to make the call, default call()).  Returns the
    errors: heal_helpers.run_heal's standard, the totals, the workspace's
    tail and, with `reference`, objs / parity / unhealed byte for byte equal
    to a device.heal run on clones of the damaged arenas."""
    n, g = case.n, case.guard
    nobj = n if nobj is None else nobj
    work, par, want, par_want = damaged(gpu, case, masks, nobj)
    ref_work, ref_par = (work.clone(), par.clone()) if reference else (None, None)
    buf = Buffers(gpu, masks)
    if invoke is None:
        out = call(le, case, work, par, buf, nobj=nobj)
        assert out[0].data_ptr() == buf.unhealed[1:1 + n].data_ptr()
        assert out[1].data_ptr() == buf.totals[1:3].data_ptr()
    else:
        invoke(work, par, buf)
    gpu.cuda.synchronize()
    ctx = f"heal_ws {case.ident()} bs {case.bs} nobj {nobj}"
    errors = check_words(gpu, case, masks, buf, nobj, ctx)
    for err in (H.arena_diff(gpu, work, want, g, f"{ctx}: objs"),
                H.arena_diff(gpu, par, par_want, 1, f"{ctx}: parity")):
        if err:
            errors.append(err)
    if reference:
        ref_un = gpu.full((n,), HH.PREFILL, dtype=gpu.int32, device="cuda")
        le.device.heal(case.cls, case.params, ref_work[g:g + n], case.size, ref_par[1:1 + n],
                       buf.lost, nobj=nobj, unhealed=ref_un)
        gpu.cuda.synchronize()
        if u32(ref_un) != u32(buf.unhealed)[1:-1]:
            errors.append(f"{ctx}: unhealed differs from heal's")
        for err in (H.arena_diff(gpu, work, ref_work, g, f"{ctx}: objs against heal's"),
                    H.arena_diff(gpu, par, ref_par, 1, f"{ctx}: parity against heal's")):
            if err:
                errors.append(err)
    return errors


def mask_case(le, oracle, cfg, B, masks):
    """One object per mask, each with its own bytes, at size k B - 1: blocks of
    B bytes, the last data block one byte short."""
    cls, k, m, w = cfg
    return H.edge_case(le, oracle, cfg, k * B - 1, n=len(masks))


def resident(cls, w):
    """Workgroups of the rebuild kernel a compute unit holds (gfw_heal_tile.hpp,
    bit_heal_tile.hpp, restated): gfw_heal_masks 16, bit_heal_masks min(32, 160 // w)."""
    return min(32, 160 // w) if cls in ("cauchyrs", "liberation") else 16
