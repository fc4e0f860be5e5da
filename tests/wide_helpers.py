"""Shared pieces of the wide-stride tests (test_device_wide_strides.py and its
child process wide_strides_child.py): device batches of three objects whose
rows lie STRIDE = 2^32 + 48 bytes apart inside one device allocation, so that
`o * stride` crosses 2^32 and 2^33 with no large data.

Every buffer of a call is a region at a fixed byte offset of every row
(Layout): the objects at 0, the parity behind them, and for repair one region
per block and per output.  A call is described on the host by a Plan: what
every region of every row holds before the call and must hold after it (both
widened by PAD bytes on each side, the allocation's fill outside the region
proper), the small buffers (flags, lost, unhealed, report, totals, workspace
tails) before and after, and the call itself.  `execute` uploads the regions,
runs the call and compares by slices on the device; `compare` and
`compare_words` take any mapping of read-back bytes, so `simulate` can feed
them what a kernel that kept a row offset or a stride in 32 bits would have
left (its accesses to row o land `o * 48` bytes past the same region of row 0,
inside the allocation), without any such kernel being built.

The damage, the expected words and the path detection are those of the
existing helper modules (scrub_helpers' whole-block damage and its models,
scrub_dev_helpers.path, heal_helpers.bits)."""
import numpy as np

import gpu_helpers as H
import heal_helpers as P
import locate_helpers as L
import locate_ws_helpers as W
import scrub_dev_helpers as D
import scrub_helpers as S
import verify_helpers as V

STRIDE = 2**32 + 48     # bytes between rows: kept in 32 bits it becomes 48
NOBJ = 3                # row offsets 0, STRIDE, 2 STRIDE: past 2^32 and past 2^33
FILL = H.GUARD_FILL     # every byte of the allocation outside the regions
PAD = 4096              # bytes compared on each side of a region
GAP = 64 << 10          # least fill between two regions
CAP = 13 * 10**9        # bytes the allocation may take
FAMILIES = V.FAMILIES   # gpu_helpers.EDGE_FAMILIES, vandrs(20,4,8) and vandrs(6,5,8)
RAGGED = 17             # size = k B - RAGGED

family_id = V.family_id

# the small per-object buffers: word 0 and word n + 1 are sentinels
PER_OBJECT = ("flags", "lost", "unhealed", "report")


def size_of(family):
    cls, k, m, w, B = family
    return k * B - RAGGED


def truncations():
    """Where an address kept in 32 bits puts row o, as a byte offset from row
    0: the product truncated, and the stride truncated before the product."""
    return [("offset", lambda o: (o * STRIDE) % 2**32), ("stride", lambda o: o * (STRIDE % 2**32))]


# ---------------------------------------------------------------------------
# Which calls serve a family (pure; the case-table test holds it against the
# library's own statuses).

def verify_fused(family):
    return V.fused(*family[:4])


def located(family):
    return L.served(*family[:4])


def located_ws(family):
    """Class (b) of leoec_locate_ws_dev."""
    return not located(family) and W.served(*family[:4])


def scrubbed_ws(family):
    """Class (b) of leoec_scrub_ws_dev."""
    return located_ws(family) and family[1] + family[2] <= 31


def healed(family):
    return family[1] + family[2] <= 32


CHILD_KINDS = ("heal", "scrub", "scrub_ws")  # run in one fresh process (the table caches)


def calls(family):
    """[(kind, variant)] of every call that serves the family."""
    cls, k, m, w, B = family
    out = [("encode", "")]
    out += [("decode", str(i)) for i in range(len(erasures(family)))]
    out += [("repair", str(i)) for i in range(len(H.edge_repairs(k, m)))]
    out += [("verify", "fused")] if verify_fused(family) else [("verify", "query"), ("verify", "one")]
    if healed(family):
        out.append(("heal", ""))
    if located(family):
        out += [("locate", ""), ("scrub", "")]
    if located_ws(family):
        out += [("locate_ws", "query"), ("locate_ws", "one")]
    if scrubbed_ws(family):
        out += [("scrub_ws", "query"), ("scrub_ws", "min")]
    return out


def case_ids(kinds):
    """The ids of every family x call of the given kinds."""
    return sorted(f"{family_id(f)}:{kind}:{var}" for f in FAMILIES for kind, var in calls(f)
                  if kind in kinds)


def erasures(family):
    """The first two sets of gpu_helpers.edge_erasures: the last m data blocks;
    the first and the last data block plus coding blocks."""
    return H.edge_erasures(family[1], family[2])[:2]


def verify_blocks(case):
    """The damaged block of each object for verify: object 0 clean, a coding
    block of object 1, the ragged last data block of object 2."""
    return [None, case.k + case.m - 1, case.k - 1]


def locate_blocks(case):
    """For locate and scrub: object 0 clean, the ragged last data block of
    object 1, the first coding block of object 2."""
    return [None, case.k - 1, case.k]


def heal_masks(case):
    """Object 0 clean, a data and a coding block of object 1, the last m data
    blocks of object 2."""
    k, m = case.k, case.m
    return [0, P.bits([0, k]), P.bits(range(k - m, k))]


# ---------------------------------------------------------------------------
# The regions of a family's rows.

def _up(x, a):
    return (x + a - 1) // a * a


class Layout:
    """name -> (byte offset in the row, length) of every region of a family:
    "objs" (the object and the row's own bytes behind it), "parity", "blk<b>"
    for each of the k + m blocks and "out<i>" for each of m repair outputs.
    Offsets are multiples of 16; every one but the first is no multiple of
    4,096; at least GAP bytes of fill lie between two regions."""

    def __init__(self, family, bs):
        cls, k, m, w, B = family
        self.family, self.bs, self.size = family, bs, size_of(family)
        self.objs_cols = _up(self.size, 16) + 32  # gpu_helpers.EdgeCase's row
        spans = [("objs", self.objs_cols), ("parity", m * bs)]
        spans += [(f"blk{b}", bs) for b in range(k + m)] + [(f"out{i}", bs) for i in range(m)]
        self.regions, end = {}, 0
        for i, (name, length) in enumerate(spans):
            off = 0 if i == 0 else _up(end, 4096) + GAP + 16 * i
            self.regions[name] = (off, length)
            end = off + length
        self.used = _up(end + PAD, 16)  # bytes of a row the family touches or compares

    def off(self, name):
        return self.regions[name][0]

    def widened(self, name):
        """(first byte, end) of the region with PAD on each side, clipped to the row."""
        off, length = self.regions[name]
        return max(off - PAD, 0), min(off + length + PAD, STRIDE)

    def blank(self, name):
        lo, hi = self.widened(name)
        return np.full(hi - lo, FILL, dtype=np.uint8)

    def put(self, image, o, name, at, data):
        """Write `data` at byte `at` of the region in the widened image."""
        start = self.off(name) - self.widened(name)[0] + at
        assert 0 <= start and start + len(data) <= len(image[(o, name)])
        image[(o, name)][start:start + len(data)] = data

    def xor(self, image, o, name, at, data):
        start = self.off(name) - self.widened(name)[0] + at
        image[(o, name)][start:start + len(data)] ^= data


def layout(le, family):
    bs, _ = le.layout(family[0], family[1:4], size_of(family))
    return Layout(family, bs)


def arena_used(le):
    """Bytes of row 2 the allocation holds: the most any family uses."""
    return max(layout(le, f).used for f in FAMILIES)


def arena_bytes(le):
    return (NOBJ - 1) * STRIDE + arena_used(le)


_cases = {}


def wide_case(le, oracle, family):
    """The family's gpu_helpers.EdgeCase of three objects (random data, random
    non-zero bytes behind `size`, the oracle's blocks), computed once."""
    if family not in _cases:
        _cases[family] = H.EdgeCase(le, oracle, family[:4], size_of(family), NOBJ)
    return _cases[family]


class Arena:
    """The device allocation: rows 0 and 1 whole and `used` bytes of row 2,
    filled with FILL once."""

    def __init__(self, gpu, used):
        self.gpu, self.used = gpu, used
        self.buf = gpu.empty((NOBJ - 1) * STRIDE + used, dtype=gpu.uint8, device="cuda")
        for lo in range(0, self.buf.numel(), 1 << 30):
            self.buf[lo:lo + (1 << 30)].fill_(FILL)

    def rows(self, off, cols):
        """[NOBJ, cols] view of a region, stride(0) == STRIDE."""
        assert off + cols <= self.used
        return self.gpu.as_strided(self.buf, (NOBJ, cols), (STRIDE, 1), off)

    def span(self, o, lo, hi):
        assert 0 <= lo <= hi <= (STRIDE if o < NOBJ - 1 else self.used)
        return self.buf[o * STRIDE + lo:o * STRIDE + hi]

    def reset(self):
        """FILL over every byte of every row a family can have touched."""
        for o in range(NOBJ):
            self.span(o, 0, self.used).fill_(FILL)

    def release(self):
        self.buf = None
        self.gpu.cuda.empty_cache()


# ---------------------------------------------------------------------------
# Plans.

class Plan:
    """One call: `pre` and `want`, {(row, region): widened bytes} before and
    after; `words_pre` and `words_want`, {name: [words]} of the small buffers;
    `outputs`, [(row, region, byte of the region, bytes)] the call writes;
    `run(gpu, le, arena, words)`, which makes the call with the small buffers
    uploaded and returns them read back; `model(objs)`, the small buffers from
    {o: (data bytes, [m coding blocks])} as a kernel read them (None: they do
    not depend on the rows)."""

    def __init__(self, case, lay, kind, variant):
        self.case, self.lay, self.kind, self.variant = case, lay, kind, variant
        self.pre, self.want, self.outputs = {}, {}, []
        self.words_pre, self.words_want = {}, {}
        self.run = self.model = None
        self.info = {}

    def ident(self):
        return f"{family_id(self.lay.family)}:{self.kind}:{self.variant}"


def _base(lay, case, parity=True):
    """Every row's objs region (the object and its own bytes behind it) and
    parity region (the oracle's coding blocks, or fill)."""
    img = {}
    for o in range(NOBJ):
        img[(o, "objs")], img[(o, "parity")] = lay.blank("objs"), lay.blank("parity")
        lay.put(img, o, "objs", 0, case.rows[o])
        if parity:
            lay.put(img, o, "parity", 0, case.parity[o])
    return img


def _copy(img):
    return {key: a.copy() for key, a in img.items()}


def _views(arena, lay, case):
    return (arena.rows(lay.off("objs"), lay.objs_cols),
            arena.rows(lay.off("parity"), case.m * case.bs))


def _i32(gpu, words):
    return gpu.from_numpy(np.array(words, dtype=np.uint32).view(np.int32).copy()).cuda()


def _poison(lay, case, img, o, b):
    """Poison block b of object o (a data block up to `size`); returns the
    output entry that puts it back, or None for a block with no valid byte."""
    where, lo, hi = S.whole_span(case, b)
    if lo >= hi:
        return None
    good = (case.rows[o, lo:hi] if where == "objs" else case.parity[o, lo:hi]).copy()
    lay.put(img, o, where, lo, np.full(hi - lo, H.POISON, dtype=np.uint8))
    return (o, where, lo, good)


def _damage(lay, case, img, blocks):
    """scrub_helpers' whole-block damage of `blocks` applied to an image;
    returns the output entries of a rebuild."""
    outputs = []
    for b, (objects, values) in S.whole_values(case, blocks).items():
        where, lo, hi = S.whole_span(case, b)
        for o, x in zip(objects, values):
            lay.xor(img, o, where, lo, x)
            good = case.rows[o, lo:hi] if where == "objs" else case.parity[o, lo:hi]
            outputs.append((o, where, lo, good.copy()))
    return outputs


def plan_encode(le, oracle, case, lay):
    p = Plan(case, lay, "encode", "")
    p.pre, p.want = _base(lay, case, parity=False), _base(lay, case)
    p.outputs = [(o, "parity", 0, case.parity[o].copy()) for o in range(NOBJ)]

    def run(gpu, le, arena, words):
        objs, par = _views(arena, lay, case)
        le.device.encode(case.cls, case.params, objs, case.size, par)
        return {}
    p.run = run
    return p


def plan_decode(le, oracle, case, lay, index):
    erased = erasures(lay.family)[index]
    p = Plan(case, lay, "decode", str(index))
    p.want = _base(lay, case)
    for o in range(NOBJ):  # an erased coding block is no survivor: never read, never written
        for e in erased:
            if e >= case.k:
                _poison(lay, case, p.want, o, e)
    p.pre = _copy(p.want)
    for o in range(NOBJ):
        for e in erased:
            if e < case.k:
                out = _poison(lay, case, p.pre, o, e)
                if out:
                    p.outputs.append(out)
    assert p.outputs
    p.info["erased"] = erased

    def run(gpu, le, arena, words):
        objs, par = _views(arena, lay, case)
        le.device.decode(case.cls, case.params, objs, case.size, par, list(erased))
        return {}
    p.run = run
    return p


def plan_repair(le, oracle, case, lay, index):
    k, m, bs = case.k, case.m, case.bs
    lost = H.edge_repairs(k, m)[index]
    p = Plan(case, lay, "repair", str(index))
    for o in range(NOBJ):
        for b in range(k + m):
            p.pre[(o, f"blk{b}")] = lay.blank(f"blk{b}")
            if b not in lost:
                lay.put(p.pre, o, f"blk{b}", 0, case.blocks[b, o])
        for i in range(m):
            p.pre[(o, f"out{i}")] = lay.blank(f"out{i}")
    p.want = _copy(p.pre)
    for o in range(NOBJ):
        for i, b in enumerate(lost):
            lay.put(p.want, o, f"out{i}", 0, case.blocks[b, o])
            p.outputs.append((o, f"out{i}", 0, case.blocks[b, o].copy()))
    p.info["lost"] = lost

    def run(gpu, le, arena, words):
        blocks = [None if b in lost else arena.rows(lay.off(f"blk{b}"), bs) for b in range(k + m)]
        outs = [arena.rows(lay.off(f"out{i}"), bs) for i in range(len(lost))]
        le.device.repair(case.cls, case.params, blocks, bs, list(lost), outs, NOBJ)
        return {}
    p.run = run
    return p


def _sentinels(words, pair):
    return [pair[0]] + list(words) + [pair[1]]


def _workspace(gpu, need):
    """`need` bytes of D.WS_FILL and D.WS_TAIL more that no call may write."""
    return gpu.full((need + D.WS_TAIL,), D.WS_FILL, dtype=gpu.uint8, device="cuda")


def _tail(ws, need):
    return ws[need:].cpu().tolist()


WS_TAIL_WANT = [D.WS_FILL] * D.WS_TAIL


def plan_verify(le, oracle, case, lay, variant):
    """variant: "fused" (no workspace), "query" (the query's workspace: one
    pass) or "one" (m bs bytes: one object per chunk, the host's o0 * stride)."""
    m, bs = case.m, case.bs
    blocks = verify_blocks(case)
    p = Plan(case, lay, "verify", variant)
    p.pre = _base(lay, case)
    _damage(lay, case, p.pre, blocks)
    p.want = _copy(p.pre)
    flags = S.flags_of(oracle, case, S.whole_objects(case, blocks))
    # what the damage means (every code here is MDS), which the oracle must agree with
    assert flags == [0, 1 << (m - 1), (1 << m) - 1], (case.ident(), flags)
    p.words_pre = {"flags": _sentinels([V.PREFILL] * NOBJ, V.SENTINELS)}
    p.words_want = {"flags": _sentinels(flags, V.SENTINELS)}
    need = le.device.verify_workspace(case.cls, case.params, case.size, NOBJ)
    assert (need == 0) == (variant == "fused") and need in (0, NOBJ * m * bs)
    need = m * bs if variant == "one" else need
    if need:
        p.words_want["workspace tail"] = WS_TAIL_WANT
    p.model = lambda objs: {"flags": _sentinels(S.flags_of(oracle, case, objs), V.SENTINELS)}

    def run(gpu, le, arena, words):
        objs, par = _views(arena, lay, case)
        fl = _i32(gpu, words["flags"])
        ws = _workspace(gpu, need) if need else None
        le.device.verify(case.cls, case.params, objs, case.size, par, flags=fl[1:1 + NOBJ],
                         workspace=None if ws is None else ws[:need])
        gpu.cuda.synchronize()
        out = {"flags": D._u32(fl)}
        if need:
            out["workspace tail"] = _tail(ws, need)
        return out
    p.run = run
    return p


def _locate_words(le, oracle, case, blocks):
    """The words the damage means, which the host model must agree with."""
    want = S.whole_words(case, blocks)
    model = S.words_of(oracle, le, case, S.whole_objects(case, blocks))
    assert [model[o] for o in range(NOBJ)] == want, (case.ident(), model, want)
    return want


def _words_model(le, oracle, case):
    return lambda objs: [S.words_of(oracle, le, case, objs)[o] for o in range(NOBJ)]


def plan_locate(le, oracle, case, lay, kind, variant):
    """kind "locate" (variant ""), or "locate_ws" with the query's workspace
    ("query") or one object's ("one")."""
    m, bs = case.m, case.bs
    blocks = locate_blocks(case)
    p = Plan(case, lay, kind, variant)
    p.pre = _base(lay, case)
    _damage(lay, case, p.pre, blocks)
    p.want = _copy(p.pre)
    want = _locate_words(le, oracle, case, blocks)
    p.words_pre = {"lost": _sentinels([L.PREFILL] * NOBJ, L.SENTINELS)}
    p.words_want = {"lost": _sentinels(want, L.SENTINELS)}
    need = 0
    if kind == "locate_ws":
        need = le.device.locate_ws_workspace(case.cls, case.params, case.size, NOBJ)
        assert need == NOBJ * m * bs
        need = m * bs if variant == "one" else need
        p.words_want["workspace tail"] = WS_TAIL_WANT
    words = _words_model(le, oracle, case)
    p.model = lambda objs: {"lost": _sentinels(words(objs), L.SENTINELS)}

    def run(gpu, le, arena, words):
        objs, par = _views(arena, lay, case)
        lost = _i32(gpu, words["lost"])
        if kind == "locate":
            le.device.locate(case.cls, case.params, objs, case.size, par, lost=lost[1:1 + NOBJ])
            gpu.cuda.synchronize()
            return {"lost": D._u32(lost)}
        ws = _workspace(gpu, need)
        le.device.locate_ws(case.cls, case.params, objs, case.size, par, lost=lost[1:1 + NOBJ],
                            workspace=ws[:need])
        gpu.cuda.synchronize()
        return {"lost": D._u32(lost), "workspace tail": _tail(ws, need)}
    p.run = run
    return p


def plan_heal(le, oracle, case, lay):
    masks = heal_masks(case)
    p = Plan(case, lay, "heal", "")
    p.want = _base(lay, case)
    p.pre = _copy(p.want)
    for o, mask in enumerate(masks):
        assert P.recoverable(mask, case.k, case.m)
        for b in P.ids_of(mask):
            out = _poison(lay, case, p.pre, o, b)
            if out:
                p.outputs.append(out)
    assert not any(o == 0 for o, _, _, _ in p.outputs)
    p.words_pre = {"masks": masks, "unhealed": _sentinels([P.PREFILL] * NOBJ, P.SENTINELS)}
    p.words_want = {"masks": masks, "unhealed": _sentinels([0] * NOBJ, P.SENTINELS)}
    p.info["masks"] = masks

    def run(gpu, le, arena, words):
        objs, par = _views(arena, lay, case)
        lost, unhealed = _i32(gpu, words["masks"]), _i32(gpu, words["unhealed"])
        le.device.heal(case.cls, case.params, objs, case.size, par, lost,
                       unhealed=unhealed[1:1 + NOBJ])
        gpu.cuda.synchronize()
        return {"masks": D._u32(lost), "unhealed": D._u32(unhealed)}
    p.run = run
    return p


def _totals(words):
    return [sum(1 for x in words if x not in (0, L.MANY)), sum(1 for x in words if x == L.MANY)]


def plan_scrub(le, oracle, case, lay, kind, variant):
    """kind "scrub" (variant ""), or "scrub_ws" with the query's workspace
    ("query") or the minimum ("min": room for one object's coding blocks).
    The contract is locate + heal's: report as locate's words, the named
    blocks rebuilt (here: back to the oracle's bytes), the totals counted.
    After run(), info["path"] is scrub_dev_helpers.path of the workspace."""
    blocks = locate_blocks(case)
    p = Plan(case, lay, kind, variant)
    p.want = _base(lay, case)
    p.pre = _copy(p.want)
    p.outputs = _damage(lay, case, p.pre, blocks)
    want = _locate_words(le, oracle, case, blocks)
    assert _totals(want) == [2, 0]
    p.words_pre = {"report": _sentinels([L.PREFILL] * NOBJ, L.SENTINELS),
                   "totals": _sentinels([D.TOTALS_PREFILL] * 2, L.SENTINELS)}
    p.words_want = {"report": _sentinels(want, L.SENTINELS),
                    "totals": _sentinels(_totals(want), L.SENTINELS),
                    "workspace tail": WS_TAIL_WANT}
    if kind == "scrub":
        need = le.device.scrub_workspace(case.cls, case.params, case.size, NOBJ)
        assert need == D.head(NOBJ)
    else:
        need = D.SCRUB_WS.workspace_bytes(le, case, 1 if variant == "min" else None)
    words = _words_model(le, oracle, case)

    def model(objs):
        rep = words(objs)
        return {"report": _sentinels(rep, L.SENTINELS), "totals": _sentinels(_totals(rep), L.SENTINELS),
                "workspace tail": WS_TAIL_WANT}
    p.model = model

    def run(gpu, le, arena, words):
        objs, par = _views(arena, lay, case)
        report, totals = _i32(gpu, words["report"]), _i32(gpu, words["totals"])
        ws = _workspace(gpu, need)
        call = le.device.scrub if kind == "scrub" else le.device.scrub_ws
        call(case.cls, case.params, objs, case.size, par, report=report[1:1 + NOBJ],
             totals=totals[1:3], workspace=ws[:need])
        gpu.cuda.synchronize()
        # one chunk holds the batch, or (minimum workspace) its last object alone
        p.info["path"] = D.path(gpu, ws, want[-1:] if variant == "min" else want)
        return {"report": D._u32(report), "totals": D._u32(totals), "workspace tail": _tail(ws, need)}
    p.run = run
    return p


def plan(le, oracle, family, kind, variant):
    case, lay = wide_case(le, oracle, family), layout(le, family)
    assert case.bs == lay.bs and case.stride == lay.objs_cols
    if kind == "encode":
        return plan_encode(le, oracle, case, lay)
    if kind == "decode":
        return plan_decode(le, oracle, case, lay, int(variant))
    if kind == "repair":
        return plan_repair(le, oracle, case, lay, int(variant))
    if kind == "verify":
        return plan_verify(le, oracle, case, lay, variant)
    if kind in ("locate", "locate_ws"):
        return plan_locate(le, oracle, case, lay, kind, variant)
    if kind == "heal":
        return plan_heal(le, oracle, case, lay)
    assert kind in ("scrub", "scrub_ws"), kind
    return plan_scrub(le, oracle, case, lay, kind, variant)


# ---------------------------------------------------------------------------
# Comparing.

def compare(lay, got, want):
    """Every (row, region) of `want` against the bytes read back (numpy arrays,
    or device tensors, which are compared on the device); the errors, each
    naming its row."""
    errors = []
    for o, name in sorted(want):
        g, w = got[(o, name)], want[(o, name)]
        lo, hi = lay.widened(name)
        if len(g) != len(w) or len(w) != hi - lo:
            errors.append(f"row {o} region {name}: {len(g)} bytes read back, {len(w)} expected")
            continue
        if not isinstance(g, np.ndarray):
            import torch
            w = torch.from_numpy(w).to(g.device)
        ne = g != w
        if not bool(ne.any()):
            continue
        first = int(ne.nonzero()[0][0])
        off = lay.off(name)
        errors.append(f"row {o} region {name} (row bytes {off}..{off + lay.regions[name][1]}): "
                      f"{int(ne.sum())} bytes differ; first at row byte {lo + first} (region byte "
                      f"{lo + first - off}): got 0x{int(g[first]):02X}, expected 0x{int(w[first]):02X}")
    return errors


def compare_words(got, want):
    """Every small buffer, whole; a per-object buffer's error names its rows."""
    errors = []
    for name in sorted(want):
        g, w = list(got.get(name, [])), list(want[name])
        if g == w:
            continue
        if name in PER_OBJECT and len(g) == len(w):
            for i in [i for i in range(len(w)) if g[i] != w[i]]:
                who = f"row {i - 1}" if 1 <= i <= NOBJ else "sentinel"
                errors.append(f"{name}: {who}: got {g[i]:#x}, expected {w[i]:#x}")
        else:
            errors.append(f"{name}: got {[hex(x) for x in g[:16]]}, expected {[hex(x) for x in w[:16]]}")
    return errors


def execute(gpu, le, arena, p):
    """Upload the plan's regions over a freshly filled arena, make the call,
    compare every region by slices on the device and every small buffer."""
    lay = p.lay
    arena.reset()
    for (o, name), a in p.pre.items():
        lo, hi = lay.widened(name)
        arena.span(o, lo, hi).copy_(gpu.from_numpy(a))
    words = p.run(gpu, le, arena, p.words_pre)
    gpu.cuda.synchronize()
    got = {(o, name): arena.span(o, *lay.widened(name)) for o, name in p.want}
    return [f"{p.ident()}: {e}" for e in compare(lay, got, p.want) + compare_words(words, p.words_want)]


def simulate(p, trunc):
    """(regions, small buffers) as a kernel leaves them whose address of row o
    is `trunc(o)` bytes past row 0 instead of o * STRIDE: every output lies at
    that displacement in row 0's region, rows 1 and 2 keep what they held, and
    the small buffers are the plan's model over what such a kernel reads."""
    lay, case = p.lay, p.case
    got = _copy(p.pre)
    for o, name, at, data in p.outputs:
        d = trunc(o)
        assert d < PAD and (d == 0) == (o == 0)
        lay.put(got, 0, name, at + d, data)
    words = {name: list(w) for name, w in p.words_want.items()}
    if p.model is not None:
        objs = {}
        for o in range(NOBJ):
            d = trunc(o)
            base = lay.off("parity") - lay.widened("parity")[0] + d
            par = p.pre[(0, "parity")]
            objs[o] = (p.pre[(0, "objs")][d:d + case.size].copy(),
                       [par[base + i * case.bs:base + (i + 1) * case.bs].copy() for i in range(case.m)])
        words.update(p.model(objs))
    return got, words
