"""The compiled instances of the packet, word and liberation kernel families
of the product library, a model of which of them a device call launches, and
the configurations test_kernel_instances.py runs so that every reachable one
runs once against the oracle.  Pure Python: no GPU, no torch, no library.

An instance is (family, template arguments):

  ("gfbit_apply", W, R, LW, ACC)   cauchyrs, w = 2..16 (gfbit_inst.hip pick())
  ("gfs_apply", W, R, ACC)         vandrs, w = 16 / 32 (gfs_inst.hip gfs_pick())
  ("libb_dec_apply", W, K, LA)     liberation decode / repair, w <= 13
  ("libb_apply", W, K)             liberation encode, w = 11, 13
  ("lib_apply", W)                 liberation encode, w = 3, 5, 7
  ("bit_apply", RO, ACC)           the generic bitmatrix kernel

The model follows the launchers: engine.cpp build_plan / run_plan (which plan
a class takes; lib_dec_plan's refusals), gfbit_inst.hip launch / pick,
kernels.hip launch(GfApply), launch(BitApply), launch(LibDecApply) and
is_liberation_encode, gfs_inst.hip gfs_pick.  Output rows go kMaxR = 4 to a
launch and input blocks kMaxK = 16; the input chunks after the first
accumulate (ACC); bit_apply takes kMaxPk / w output blocks per pass and its
RO is the packet count of the pass rounded up to even.  The output rows of a
decode are the erased data blocks that start below `size` (at most m); those
of a repair are the ids the caller names, which leoec_repair_dev neither
bounds by m nor requires to be absent."""

kMaxK, kMaxR, kMaxPk = 16, 4, 32
LIB_WS = (3, 5, 7, 11, 13)        # liberation widths with kernels of their own
kLibbEncMinW = 11                  # liberation encode: libb_apply from here
GFBIT_WS = tuple(range(2, 17))


def gfbit_lw(w):
    """gfbit_apply's lane width in dwords (gfbit_w.hip)."""
    return 1 if w >= 12 else 2


def libb_dec_la(w, k):
    """libb_dec_apply's look-ahead (kernels_impl.hpp)."""
    return 4 if (w >= 13 or k <= 4) else 2


def block_size(k, w, size):
    """engine.cpp op_layout, the same for every class."""
    kw = k * w
    return -(-(-(-size // kw)) // 16) * 16 * w


def _chunks(total, per):
    """[(start, count)] of `total` items taken `per` at a time."""
    return [(s, min(per, total - s)) for s in range(0, total, per)]


def survivors(k, m, gone):
    """op_decode_dev / op_repair_dev: the first k ids that are not gone."""
    return [b for b in range(k + m) if b not in gone][:k]


def lib_dec_serves(k, surv, want):
    """engine.cpp lib_dec_plan: False where it answers LEOEC_E_UNSUPPORTED
    and the generic bitmatrix path takes the plan."""
    if not 1 <= len(want) <= 2:
        return False
    e = [j for j in range(k) if j not in surv]
    c = [r for r in range(2) if k + r in surv]
    if len(e) != len(c):
        return False
    if any(b in surv for b in want):
        return False
    if not e and len(want) == 2:  # the encode
        return False
    return True


def wanted(k, m, w, op, ids, size):
    """(survivor ids, wanted ids) of a device call.  op "encode": ids unused;
    "decode": ids are the erased ones and only the erased data blocks that
    start below `size` are rebuilt; "repair": ids are the lost (absent) ones,
    all rebuilt; "refresh": every block present, ids recomputed.
    leoec_repair_dev bounds neither the number of wanted ids nor asks that
    they be absent (op_repair_dev: any ids below k + m, duplicates included),
    so repair's R is not bounded by m: "refresh" stands for those calls."""
    if op == "encode":
        return list(range(k)), list(range(k, k + m))
    if op == "decode":
        bs = block_size(k, w, size)
        return survivors(k, m, ids), [b for b in sorted(set(ids)) if b < k and b * bs < size]
    if op == "repair":
        return survivors(k, m, ids), list(ids)
    if op == "refresh":
        return list(range(k)), list(ids)
    raise ValueError(op)


def _bit_apply(k, w, nwant):
    out = set()
    for _, nb in _chunks(nwant, kMaxPk // w):
        ro = (nb * w + 1) // 2 * 2
        for j0, _ in _chunks(k, kMaxK):
            out.add(("bit_apply", ro, j0 > 0))
    return out


def instances(cls, k, m, w, op, ids=(), size=1 << 40):
    """The set of kernel instances the device call launches (launches below
    gfbk_apply's 4 GB threshold).  ids / size: see wanted(); the default size
    makes every data block non-empty."""
    surv, want = wanted(k, m, w, op, list(ids), size)
    nwant = len(want)
    if nwant == 0:
        return set()
    grid = [(nr, j0 > 0) for _, nr in _chunks(nwant, kMaxR) for j0, _ in _chunks(k, kMaxK)]
    if cls == "vandrs" and w in (16, 32):
        return {("gfs_apply", w, nr, acc) for nr, acc in grid}
    if cls == "cauchyrs" and w in GFBIT_WS:
        return {("gfbit_apply", w, nr, gfbit_lw(w), acc) for nr, acc in grid}
    if cls == "cauchyrs":
        return _bit_apply(k, w, nwant)
    if cls == "liberation":
        if w in LIB_WS:
            if lib_dec_serves(k, surv, want):
                return {("libb_dec_apply", w, k, libb_dec_la(w, k))}
            if op == "encode" or (surv == list(range(k)) and want == [k, k + 1]):
                # is_liberation_encode: the coding bitmatrix itself, P then Q
                return {("libb_apply", w, k)} if w >= kLibbEncMinW else {("lib_apply", w)}
        return _bit_apply(k, w, nwant)
    raise ValueError((cls, w))


# ---------------------------------------------------------------------------
# What the product library compiles (the inventory test reads the same from
# the kernel names of the built objects).

def inventory():
    inv = set()
    for w in GFBIT_WS:
        inv |= {("gfbit_apply", w, r, gfbit_lw(w), acc) for r in range(1, 5) for acc in (False, True)}
    inv |= {("gfs_apply", w, r, acc) for w in (16, 32) for r in range(1, 5) for acc in (False, True)}
    inv |= {("libb_dec_apply", w, k, libb_dec_la(w, k)) for w in LIB_WS for k in range(1, w + 1)}
    inv |= {("libb_apply", w, k) for w in LIB_WS if w >= kLibbEncMinW for k in range(1, w + 1)}
    inv |= {("lib_apply", w) for w in LIB_WS}
    inv |= {("bit_apply", ro, acc) for ro in range(2, 33, 2) for acc in (False, True)}
    return inv


UNREACHABLE = {}
# cauchyrs needs k + m <= 2^w, so w <= 4 has k <= 15.  (The number of output
# rows has no such bound: leoec_repair_dev takes any number of ids, present
# blocks included, so gfbit_apply<2,4,...> runs for a repair of all four
# blocks of a w = 2 code: refreshes().)
for _w in (2, 3, 4):
    for _r in range(1, 5):
        UNREACHABLE[("gfbit_apply", _w, _r, 2, True)] = \
            "cauchyrs w = %d: k + m <= %d, never a 17th input block" % (_w, 1 << _w)
# lib_kernel_w's `if constexpr` has no else: the table entry is compiled, the
# launcher returns libb_apply before it is consulted
for _w in (11, 13):
    UNREACHABLE[("lib_apply", _w)] = "liberation w = %d encodes through libb_apply" % _w
# bit_apply below RO = 18 serves w <= 16: cauchyrs there is gfbit_apply, and
# liberation has k <= w <= 13 < 17 input blocks (no ACC) and at least 3
# packets (no RO = 2)
UNREACHABLE[("bit_apply", 2, False)] = "one output block is w >= 3 packets"
for _ro in range(2, 17, 2):
    UNREACHABLE[("bit_apply", _ro, True)] = \
        "RO <= 16 is liberation w <= 13, where k <= w < 17: one input chunk"
del _w, _r, _ro

# Outside this module's reach: covered elsewhere.
ELSEWHERE = {
    "gfbk_apply": "launches of at least 4 GB of cauchyrs(10,4,8): "
                  "test_gpu_parity.py::test_cauchy_large_launch_gfbk",
}


# ---------------------------------------------------------------------------
# Sizes.  B: one full tile of the family's shipped tile in every block (or
# packet) plus 128 bytes of the next.

# The launchers' constants this module restates, each with the place it is
# written at: (file under leo_erasure_amd/csrc, pattern, the value here).
# test_kernel_instances.py::test_constants_are_the_sources reads the files, so
# a shipped tile or chunk size that changes fails there until the numbers
# here, and with them the sizes of every configuration, follow.
kThreads, kLibLanes, kLibbEncTW, kLibbDecTW, kGfsLanes, kGfsRegs = 256, 64, 64, 64, 64, 16
SOURCE_CONSTANTS = [
    ("kernels_impl.hpp", r"constexpr int kThreads = (\d+);", kThreads),
    ("kernels_impl.hpp", r"constexpr uint32_t kTileBytes = kThreads \* (\d+);", 16),
    ("kernels_impl.hpp", r"constexpr int kMaxK = (\d+);", kMaxK),
    ("kernels_impl.hpp", r"constexpr int kMaxR = (\d+);", kMaxR),
    ("kernels_impl.hpp", r"constexpr int kMaxPk = (\d+);", kMaxPk),
    ("kernels_impl.hpp", r"kLibbEncTW = (\d+)", kLibbEncTW),
    ("kernels_impl.hpp", r"constexpr int kLibbDecTW = (\d+);", kLibbDecTW),
    ("kernels_impl.hpp", r"kLibbEncMinW = (\d+)", kLibbEncMinW),
    ("kernels_impl.hpp", r"libb_dec_la\(int w, int k\) \{ return \(w >= (\d+) \|\| k <= 4\) \? 4 : 2; \}", 13),
    ("kernels_impl.hpp", r"int WG = kThreads, int XMAP = 0, int WAVES = (\d+)>\s*__global__[^;{]*gfbit_apply", 0),
    ("kernels.hip", r"constexpr uint32_t kLibLanes = (\d+);", kLibLanes),
    ("gfs_inst.hip", r"constexpr int kGfsLanes = (\d+);", kGfsLanes),
    ("gfs_inst.hip", r"constexpr int kGfsRegs = (\d+);", kGfsRegs),
    ("gfbit_w.hip", r"constexpr int kLW = kW >= (\d+) \? 1 : 2;", 12),
]


def tile_bytes(cls, w):
    """Bytes of a block (vandrs) or of a packet per workgroup: lanes x bytes
    per lane of the shipped form."""
    if cls == "vandrs":
        return kGfsLanes * 4 * kGfsRegs           # gfs_apply: kGfsTile
    if cls == "cauchyrs" and w <= 16:
        return kThreads * 4 * gfbit_lw(w)         # gfbit_apply: WG lanes of LW dwords
    if cls == "liberation" and w in LIB_WS:
        assert kLibLanes == kLibbEncTW == kLibbDecTW
        return kLibLanes * 16                     # lib_apply, libb_apply, libb_dec_apply
    return kThreads * 16                          # bit_apply: kTileBytes


def big_block(cls, w):
    """B: a full tile and 128 bytes of the next in every packet; vandrs: in
    the block, rounded up to the multiple of 16 x 32 every w needs (4,608)."""
    t = tile_bytes(cls, w) + 128
    return -(-t // 512) * 512 if cls == "vandrs" else t * w


def sizes(cls, k, w):
    """k B - 3 (the last block 3 bytes short) and, for k >= 2,
    16 w (k - 1) + 5 (16 w-byte blocks, the last one 5 bytes)."""
    out = [k * big_block(cls, w) - 3]
    if k >= 2:
        out.append(16 * w * (k - 1) + 5)
    return out


# ---------------------------------------------------------------------------
# Operations of a configuration.

def erasures(k, m):
    """Decode: the last r data blocks (ragged output, every survivor full),
    then the first r (the ragged block a survivor), r = 1..min(k, m)."""
    out = []
    for r in range(1, min(k, m) + 1):
        for s in (list(range(k - r, k)), list(range(r))):
            if s not in out:
                out.append(s)
    return out


def edge_repairs(k, m):
    """gpu_helpers.edge_repairs(k, m), restated (this module imports no
    numpy; the no-GPU test holds the two equal for m >= 2).  m = 1 can lose
    one block: the first data block, then the coding block."""
    sets = ([k - 1, k], [0, k // 2, k, k + m - 1][:m]) if m >= 2 else ([0], [k])
    out = []
    for s in sets:
        s = sorted(set(s))
        if s not in out:
            out.append(s)
    return out


def lib_singles_and_pairs(k):
    ids = list(range(k + 2))
    return [[a] for a in ids] + [[a, b] for a in ids for b in ids if a < b]


def refreshes(cls, k, m, w):
    """Repairs of blocks that are present (leoec_repair_dev recomputes them,
    any number of them), where they are the only way to an instance:
    cauchyrs w = 2 has k + m <= 4, so gfbit_apply<2,4,...> runs only when all
    four blocks of a code with k + m = 4 are wanted; liberation w <= 13 plans
    lib_dec_plan refuses are the only product path to bit_apply<4..16>: one,
    two or three wanted blocks give RO = w, 2 w and 3 w rounded to even
    within a pass of kMaxPk / w blocks."""
    if cls == "cauchyrs" and w == 2 and k + m == 4:
        return [[0, 1, 2, 3]]
    if cls != "liberation" or w not in LIB_WS:
        return []
    out = [[0]]
    if w in (3, 5):
        out.append([0, k, k + 1])      # 9 -> 10 and 15 -> 16 packets
    return out


def operations(cls, k, m, w):
    """[(op, ids)] of one configuration, in the order the GPU test runs them."""
    ops = [("encode", [])]
    ops += [("decode", e) for e in erasures(k, m)]
    ops += [("repair", r) for r in edge_repairs(k, m)]
    if cls == "liberation" and w in LIB_WS:
        sp = lib_singles_and_pairs(k)
        ops += [("decode", e) for e in sp if ("decode", e) not in ops]
        ops += [("repair", e) for e in sp if len(e) == 2 and ("repair", e) not in ops]
    ops += [("refresh", r) for r in refreshes(cls, k, m, w)]
    return ops


# ---------------------------------------------------------------------------
# The configurations: (class, w) -> [(k, m)], one pytest parameter each.

def _cauchy_small(w):
    lim = 1 << w
    if w == 2:
        return [(k, m) for k in (1, 2, 3) for m in range(1, 4) if k + m <= lim]
    ks = [k for k in ((3, 4) if w == 3 else (4, 5, 17, 20))]
    return [(k, m) for k in ks for m in range(1, 5) if k + m <= lim]


TABLE = {}
for _w in GFBIT_WS:
    TABLE[("cauchyrs", _w)] = _cauchy_small(_w)
for _w in range(17, 33):
    # m = 2 is unsupported above w = 20 (codes.cpp, the cbest rows)
    TABLE[("cauchyrs", _w)] = [(k, m) for k in (3, 17) for m in (1, 3)]
for _w in (16, 32):
    TABLE[("vandrs", _w)] = [(k, m) for k in list(range(1, 19)) + [20] for m in range(1, 5)]
for _w in LIB_WS:
    TABLE[("liberation", _w)] = [(k, 2) for k in range(1, _w + 1)]
for _w in (17, 19, 23, 29, 31):
    TABLE[("liberation", _w)] = [(k, 2) for k in sorted({2, 17, _w})]
del _w


def configs():
    """[(class, k, m, w)] of the whole table."""
    return [(cls, k, m, w) for (cls, w), kms in TABLE.items() for k, m in kms]


def reached(cfgs=None):
    """{instance: a (configuration, size, op, ids) that launches it}."""
    out = {}
    for cls, k, m, w in (configs() if cfgs is None else cfgs):
        for size in sizes(cls, k, w):
            for op, ids in operations(cls, k, m, w):
                for inst in instances(cls, k, m, w, op, ids, size):
                    out.setdefault(inst, ((cls, k, m, w), size, op, ids))
    return out


# ---------------------------------------------------------------------------
# The kernels of the built objects.

FAMILY_ARGS = {
    # family -> the instance of a kernel's template arguments (the leading ones)
    "gfbit_apply": lambda a: ("gfbit_apply", a[0], a[1], a[2], bool(a[3])),
    "gfs_apply": lambda a: ("gfs_apply", a[0], a[1], bool(a[2])),
    "libb_dec_apply": lambda a: ("libb_dec_apply", a[0], a[1], a[2]),
    "libb_apply": lambda a: ("libb_apply", a[0], a[1]),
    "lib_apply": lambda a: ("lib_apply", a[0]),
    "bit_apply": lambda a: ("bit_apply", a[0], bool(a[1])),
}
# every template argument in full, to hold the arguments an instance leaves out
FULL_ARGS = {
    "gfbit_apply": lambda w, r, lw, acc: [w, r, lw, int(acc), 1, 0, 0, 256, 0, 0],
    "gfs_apply": lambda w, r, acc: [w, r, int(acc), 0, 1],
    "libb_dec_apply": lambda w, k, la: [w, k, la, 64],
    "libb_apply": lambda w, k: [w, k, 2, 64],
    "lib_apply": lambda w: [w, 2, 64],
    "bit_apply": lambda ro, acc: [ro, int(acc), 0, 2, 0],
}


def parse_kernel(name):
    """(family, [template arguments]) of a mangled kernel name of the leoec
    namespaces, or None: _ZN5leoec<len><ns><len><name>I(Li<n>E|Lb<n>E|Lj<n>E)*E..."""
    import re
    if not name.startswith("_ZN5leoec"):
        return None
    i, ident = 3, None
    while i < len(name) and name[i].isdigit():
        j = i
        while name[j].isdigit():
            j += 1
        ident, i = name[j:j + int(name[i:j])], j + int(name[i:j])
    if i >= len(name) or name[i] != "I":
        return None
    lits = re.match(r"(?:L[ibj]n?\d+E)*", name[i + 1:]).group(0)
    args = [(-1 if neg else 1) * int(v) for neg, v in re.findall(r"L[ibj](n?)(\d+)E", lits)]
    return ident, args


def built_instances(kernel_names):
    """(instances of the six families, full-argument mismatches) among kernel names."""
    found, odd = set(), []
    for name in kernel_names:
        p = parse_kernel(name)
        if p is None or p[0] not in FAMILY_ARGS:
            continue
        inst = FAMILY_ARGS[p[0]](p[1])
        found.add(inst)
        if FULL_ARGS[p[0]](*inst[1:]) != p[1]:
            odd.append((name, p[1]))
    return found, odd
