"""Every compiled instance of the packet, word and liberation kernel families
of the product library, run once against the oracle.

gfbit_apply<W,R,LW,ACC> (cauchyrs w = 2..16), gfs_apply<W,R,ACC> (vandrs
w = 16 / 32), libb_dec_apply<W,K> / libb_apply<W,K> / lib_apply<W>
(liberation w <= 13) and bit_apply<RO,ACC> (everything at w >= 17) put their
straight-line code behind template arguments: one polynomial per width, one
unrolled body per (w, k), one edge path per lane width, accumulating forms
that re-read their own outputs.  A wrong instance is wrong alone.

instance_tables.py holds the inventory, a model of the launchers' dispatch
and the configuration table; here
  * no GPU: the model's union over the table is the inventory minus
    UNREACHABLE, the oracle and the library accept and encode every
    configuration, the sizes have the block geometry the table claims, and
    the kernel names of the built objects are exactly reached + UNREACHABLE;
  * GPU: per configuration and size, on the edge harness of gpu_helpers
    (guard rows, random non-zero bytes behind every object, every byte of
    every arena compared with the oracle's blocks): encode; decode of the last
    r and of the first r data blocks, r = 1..min(k, m); repair of
    edge_repairs(k, m); for liberation w <= 13 every single erased id and
    every pair of the k + 2 blocks through decode and every pair through
    repair (each mbits table, each absent-shard position, wanted coding
    blocks through syndromes), and repairs of present blocks, the plans
    lib_dec_plan refuses, which are the only way to bit_apply<4..16>; for
    cauchyrs w = 2 a repair of all four blocks with every block present,
    the only way to gfbit_apply<2,4> (leoec_repair_dev bounds neither the
    number of ids nor asks that they be absent).

Two sizes per configuration: k B - 3 (one full tile of the family's shipped
tile in every block or packet and part of the next, the last block 3 bytes
short) and 16 w (k - 1) + 5 (16 w-byte blocks, the last one 5 bytes), 3
objects each.

The second half holds the scrub calls (verify, locate_ws, heal) at the limits
bit_locate is written against, with scrub_helpers' position batch, and the
sweep of bit_heal_list (leoec_scrub_ws_dev's rebuild: one instance, w, k and m
runtime values) over every w and the same limits, in child processes of at
most 16 configurations (tests/scrub_ws_instances_child.py)."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_helpers as H
import instance_tables as T
import locate_helpers as L
import locate_ws_helpers as W
import scrub_helpers as S
import scrub_ws_instances_child as BC
import test_code_objects as CO

E_UNSUPPORTED = -14
MAX_OPS = 400  # device calls of one pytest parameter, about


def _ops(cfg):
    cls, k, m, w = cfg
    return len(T.sizes(cls, k, w)) * len(T.operations(cls, k, m, w))


def _groups():
    """[(class, w, [(k, m)])]: the table cut into parameters of at most about
    MAX_OPS device calls (liberation w <= 13: one per k)."""
    out = []
    for (cls, w), kms in T.TABLE.items():
        cur, n = [], 0
        for k, m in kms:
            c = _ops((cls, k, m, w))
            if cur and (n + c > MAX_OPS or (cls == "liberation" and w in T.LIB_WS)):
                out.append((cls, w, cur))
                cur, n = [], 0
            cur.append((k, m))
            n += c
        out.append((cls, w, cur))
    return out


GROUPS = _groups()


def _gid(g):
    cls, w, kms = g
    ks = sorted({k for k, _ in kms})
    return "%s-w%d-k%s" % (cls, w, ks[0] if len(ks) == 1 else "%d..%d" % (ks[0], ks[-1]))


# ---------------------------------------------------------------------------
# No GPU.

def test_dispatch_model():
    """The model on plans read off the launchers by hand."""
    I = T.instances
    # cauchyrs w <= 16: gfbit_apply, 4 rows and 16 inputs per launch
    assert I("cauchyrs", 10, 4, 8, "encode") == {("gfbit_apply", 8, 4, 2, False)}
    assert I("cauchyrs", 20, 3, 13, "encode") == {("gfbit_apply", 13, 3, 1, False),
                                                  ("gfbit_apply", 13, 3, 1, True)}
    assert I("cauchyrs", 5, 6, 8, "encode") == {("gfbit_apply", 8, 4, 2, False),
                                                ("gfbit_apply", 8, 2, 2, False)}
    # decode's R: erased data blocks that start below size (erased coding ids only pick survivors)
    assert I("cauchyrs", 5, 3, 8, "decode", [3, 4, 6]) == {("gfbit_apply", 8, 2, 2, False)}
    bs = T.block_size(5, 8, 128 * 3 + 5)
    assert bs == 128
    assert I("cauchyrs", 5, 3, 8, "decode", [3, 4], 128 * 3 + 5) == {("gfbit_apply", 8, 1, 2, False)}
    assert I("cauchyrs", 5, 3, 8, "decode", [4], 128 * 3 + 5) == set()
    # repair's R: the lost ids
    assert I("vandrs", 17, 4, 32, "repair", [0, 17, 20]) == {("gfs_apply", 32, 3, False),
                                                             ("gfs_apply", 32, 3, True)}
    # cauchyrs above w = 16: bit_apply, kMaxPk / w = 1 block per pass
    assert I("cauchyrs", 17, 3, 17, "encode") == {("bit_apply", 18, False), ("bit_apply", 18, True)}
    assert I("cauchyrs", 3, 3, 32, "decode", [0, 1]) == {("bit_apply", 32, False)}
    # liberation
    assert I("liberation", 4, 2, 7, "encode") == {("lib_apply", 7)}
    assert I("liberation", 10, 2, 11, "encode") == {("libb_apply", 11, 10)}
    assert I("liberation", 10, 2, 11, "repair", [10, 11]) == {("libb_apply", 11, 10)}
    assert I("liberation", 4, 2, 7, "decode", [1, 3]) == {("libb_dec_apply", 7, 4, 4)}
    assert I("liberation", 7, 2, 7, "decode", [6, 8]) == {("libb_dec_apply", 7, 7, 2)}
    assert I("liberation", 7, 2, 7, "decode", [7, 8]) == set()
    assert I("liberation", 5, 2, 13, "repair", [5]) == {("libb_dec_apply", 13, 5, 4)}
    assert I("liberation", 17, 2, 17, "encode") == {("bit_apply", 18, False), ("bit_apply", 18, True)}
    assert I("liberation", 31, 2, 31, "decode", [0, 30]) == {("bit_apply", 32, False),
                                                             ("bit_apply", 32, True)}
    # repair takes any number of ids, present blocks included: rows beyond m
    assert I("cauchyrs", 2, 2, 2, "refresh", [0, 1, 2, 3]) == {("gfbit_apply", 2, 4, 2, False)}
    assert I("cauchyrs", 1, 3, 2, "refresh", [0, 1, 2, 3]) == {("gfbit_apply", 2, 4, 2, False)}
    assert I("cauchyrs", 4, 2, 8, "refresh", [0, 1, 2, 3, 4, 5]) == {("gfbit_apply", 8, 4, 2, False),
                                                                      ("gfbit_apply", 8, 2, 2, False)}
    # a present block recomputed: lib_dec_plan refuses, bit_apply takes it
    assert I("liberation", 3, 2, 3, "refresh", [0]) == {("bit_apply", 4, False)}
    assert I("liberation", 5, 2, 5, "refresh", [0, 5, 6]) == {("bit_apply", 16, False)}
    assert I("liberation", 7, 2, 7, "refresh", [0, 7, 8]) == {("bit_apply", 22, False)}
    assert I("liberation", 4, 2, 7, "refresh", [4, 5]) == {("lib_apply", 7)}


def test_every_reachable_instance_is_in_the_table():
    inv = T.inventory()
    assert len(inv) == 120 + 16 + 39 + 24 + 5 + 32
    assert set(T.UNREACHABLE) <= inv
    assert all(isinstance(r, str) and r for r in T.UNREACHABLE.values())
    reached = T.reached()
    assert not set(reached) & set(T.UNREACHABLE), sorted(set(reached) & set(T.UNREACHABLE))
    missing = inv - set(reached) - set(T.UNREACHABLE)
    assert not missing, sorted(missing)
    assert set(reached) <= inv, sorted(set(reached) - inv)
    # the 12 accumulating packet instances of w <= 4, the two dead lib_apply
    # entries, bit_apply<2> and the accumulating bit_apply<2..16>
    count = lambda fam: sum(1 for i in T.UNREACHABLE if i[0] == fam)  # noqa: E731
    assert (count("gfbit_apply"), count("lib_apply"), count("bit_apply")) == (12, 2, 9)
    assert len(T.UNREACHABLE) == 23
    # no repair of present blocks, however many, reaches one of them either:
    # four or five wanted ids (two passes of rows) on every configuration
    for cls, k, m, w in T.configs():
        for ids in ([0] * 4, list(range(min(k + m, 5))) + [0] * max(0, 5 - k - m)):
            got = T.instances(cls, k, m, w, "refresh", ids)
            assert not got & set(T.UNREACHABLE), (cls, k, m, w, ids)
    # the parameters are the whole table, each configuration once
    cfgs = [(cls, k, m, w) for cls, w, kms in GROUPS for k, m in kms]
    assert sorted(cfgs) == sorted(T.configs()) and len(set(cfgs)) == len(cfgs)


def test_constants_are_the_sources():
    """The chunk sizes, lane counts and thresholds instance_tables restates
    are the ones written in the launchers: the tile sizes behind every
    configuration's B follow the shipped kernels."""
    import re
    csrc = os.path.join(CO.ROOT, "leo_erasure_amd", "csrc")
    text = {}
    for name, pattern, value in T.SOURCE_CONSTANTS:
        if name not in text:
            with open(os.path.join(csrc, name)) as fh:
                text[name] = fh.read()
        found = re.findall(pattern, text[name])
        assert found == [str(value)], (name, pattern, found, value)
    assert [T.tile_bytes("cauchyrs", w) for w in (2, 11, 12, 16, 17)] == [2048, 2048, 1024, 1024, 4096]
    assert (T.tile_bytes("vandrs", 16), T.tile_bytes("liberation", 13), T.tile_bytes("liberation", 17)) \
        == (4096, 1024, 4096)
    assert [T.big_block("cauchyrs", w) // w for w in (11, 12, 17)] == [2176, 1152, 4224]
    assert (T.big_block("vandrs", 32), T.big_block("liberation", 7)) == (4608, 1152 * 7)


def test_table_is_what_it_claims():
    """The configuration lists by their stated purpose."""
    for w in T.GFBIT_WS:
        kms = T.TABLE["cauchyrs", w]
        assert all(k + m <= 1 << w for k, m in kms)
        if w == 2:
            assert sorted(kms) == [(k, m) for k in (1, 2, 3) for m in (1, 2, 3) if k + m <= 4]
            # all four blocks of (3,1), (2,2), (1,3) recomputed: the only R = 4 at w = 2
            assert [(k, m) for k, m in sorted(kms)
                    if ("refresh", [0, 1, 2, 3]) in T.operations("cauchyrs", k, m, 2)] \
                == [(1, 3), (2, 2), (3, 1)]
        elif w == 3:
            assert {k for k, _ in kms} == {3, 4} and (4, 4) in kms
        elif w == 4:
            assert {k for k, _ in kms} == {4, 5} and {m for _, m in kms} == {1, 2, 3, 4}
        else:  # both parities of the two-block ring loop; ACC with nk = 1 and 4
            assert sorted(kms) == [(k, m) for k in (4, 5, 17, 20) for m in (1, 2, 3, 4)]
    for w in (16, 32):
        assert sorted(T.TABLE["vandrs", w]) == [(k, m) for k in list(range(1, 19)) + [20]
                                                for m in (1, 2, 3, 4)]
    for w in T.LIB_WS:
        assert T.TABLE["liberation", w] == [(k, 2) for k in range(1, w + 1)]
    for cls, k, m, w in T.configs():
        assert T.edge_repairs(k, m) == (H.edge_repairs(k, m) if m >= 2 else [[0], [k]])
        assert sorted({len(e) for e in T.erasures(k, m)}) == list(range(1, min(k, m) + 1))
        if cls == "liberation" and w in T.LIB_WS:
            ops = T.operations(cls, k, m, w)
            pairs = [[a, b] for a in range(k + 2) for b in range(a + 1, k + 2)]
            assert all(("decode", [a]) in ops for a in range(k + 2))
            assert all(("decode", p) in ops and ("repair", p) in ops for p in pairs)


@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_configurations_accepted_and_sized(le, oracle, group):
    """Both sides accept every configuration and the oracle encodes a 1-byte
    object of it (check_params passes cases the matrix builder refuses); the
    sizes have the geometry the table claims; at the big size decode reaches
    every R the erasure sets ask for."""
    cls, w, kms = group
    tile = T.tile_bytes(cls, w)
    B = T.big_block(cls, w)
    unit = B if cls == "vandrs" else B // w
    assert B % (16 * w) == 0 and tile < unit < 2 * tile and (unit - tile) % 128 == 0
    for k, m in kms:
        assert oracle.check_params(cls, k, m, w) == 0, (cls, k, m, w)
        assert le.lib.leoec_check_params(le._lib.CODING_IDS[cls], k, m, w) == 0, (cls, k, m, w)
        assert len(oracle.encode(cls, k, m, w, b"\x5a")) == k + m
        szs = T.sizes(cls, k, w)
        assert len(szs) == (2 if k >= 2 else 1)
        assert le.layout(cls, (k, m, w), szs[0])[0] == B == T.block_size(k, w, szs[0])
        assert H.block_valids(k, B, szs[0])[-1] == B - 3
        for e in T.erasures(k, m):
            inst = T.instances(cls, k, m, w, "decode", e, szs[0])
            rs = {i[2] for i in inst if i[0] in ("gfbit_apply", "gfs_apply")}
            assert inst and rs in (set(), {len(e)}), (cls, k, m, w, e)
        if k >= 2:
            assert le.layout(cls, (k, m, w), szs[1])[0] == 16 * w == T.block_size(k, w, szs[1])
            assert H.block_valids(k, 16 * w, szs[1])[-2:] == [16 * w, 5]


def _have_objects():
    return bool(glob.glob(os.path.join(CO.BUILD, "*.o")))


def _have_tools():
    return bool(CO._tool("clang-offload-bundler") and CO._tool("llvm-readelf") and CO._tool("llvm-objcopy"))


def test_kernel_name_parser():
    p = T.parse_kernel
    assert p("_ZN5leoec6detail11gfbit_applyILi13ELi4ELi1ELb1ELi1ELb0ELi0ELi256ELi0ELi0EEEvNS0_7GfbArgsIXT0_EEE") \
        == ("gfbit_apply", [13, 4, 1, 1, 1, 0, 0, 256, 0, 0])
    assert p("_ZN5leoec6detail9bit_applyILi18ELb0ELb0ELi2ELi0EEEvNS0_7BitArgsE") == ("bit_apply", [18, 0, 0, 2, 0])
    assert p("_ZN5leoec6detail9lib_applyILi7ELi2ELi64EEEvNS0_7LibArgsE") == ("lib_apply", [7, 2, 64])
    assert p("_ZN5leoec12_GLOBAL__N_110bit_locateENS0_10BitLocArgsEPj") is None
    assert p("memset") is None
    found, odd = T.built_instances(["_ZN5leoec6detail9lib_applyILi7ELi2ELi64EEEvNS0_7LibArgsE",
                                    "_ZN5leoec6detail9lib_applyILi7ELi4ELi256EEEvNS0_7LibArgsE"])
    assert found == {("lib_apply", 7)} and len(odd) == 1


@pytest.mark.skipif(not _have_objects(), reason="product objects not built")
@pytest.mark.skipif(not _have_tools(), reason="ROCm LLVM tools absent")
def test_built_kernels_are_the_inventory(tmp_path):
    """The kernels of the six families in the product objects (names from the
    code objects' metadata) are exactly reached + UNREACHABLE, each in the
    shipped form of its remaining template arguments: a kernel added later
    without a row in the table fails here."""
    names = []
    for o in sorted(glob.glob(os.path.join(CO.BUILD, "*.o"))):
        try:
            names += [n for n, _ in CO.kernel_notes(o, str(tmp_path))]
        except (AssertionError, CO.subprocess.CalledProcessError):
            continue  # (an object with no device code)
    assert len(names) > 100, len(names)
    found, odd = T.built_instances(names)
    assert not odd, odd[:10]
    want = set(T.reached()) | set(T.UNREACHABLE)
    assert found == want, (sorted(found - want), sorted(want - found))
    # gfbk_apply: shipped, reached only by launches this module cannot make
    assert any((T.parse_kernel(n) or ("",))[0] == "gfbk_apply" for n in names)
    assert set(T.ELSEWHERE) == {"gfbk_apply"}


# ---------------------------------------------------------------------------
# GPU.

def check_refresh(gpu, le, case, ids):
    """Device repair of `ids` with every block present (the survivors are the
    data blocks): the oracle's blocks in [0, bs) of every output row, the
    fill everywhere else, the inputs untouched.  Returns None or the error."""
    k, m, bs, n = case.k, case.m, case.bs, case.n
    snaps = [case.arena(gpu, np.concatenate([case.blocks[b], case.slack[b]], axis=1), H.GUARD_FILL)
             for b in range(k + m)]
    work = [s.clone() for s in snaps]
    outs = [case.arena(gpu, bs + 48, H.REPAIR_FILL) for _ in ids]
    le.device.repair(case.cls, case.params, [a[1:1 + n] for a in work], bs, list(ids),
                     [o[1:1 + n] for o in outs], n)
    gpu.cuda.synchronize()
    ctx = f"{case.ident()} bs {bs} present, recomputed {list(ids)}"
    for o, b in zip(outs, ids):
        want = np.full((n, bs + 48), H.REPAIR_FILL, dtype=np.uint8)
        want[:, :bs] = case.blocks[b]
        err = H.arena_diff(gpu, o, case.arena(gpu, want, H.REPAIR_FILL), 1, f"repair {ctx}: block {b}")
        if err:
            return err
    for b in range(k + m):
        err = H.arena_diff(gpu, work[b], snaps[b], 1, f"repair {ctx}: input block {b}")
        if err:
            return err
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS, ids=_gid)
def test_kernel_instance(gpu, le, oracle, group):
    cls, w, kms = group
    errors = []
    for k, m in kms:
        for size in T.sizes(cls, k, w):
            case = H.edge_case(le, oracle, (cls, k, m, w), size, n=3)
            for op, ids in T.operations(cls, k, m, w):
                if op == "encode":
                    err = H.check_encode(gpu, le, case)
                elif op == "decode":
                    err = H.check_decode(gpu, le, case, ids)
                elif op == "repair":
                    err = H.check_repair(gpu, le, case, ids)
                else:
                    err = check_refresh(gpu, le, case, ids)
                if err:
                    errors.append(err)
    assert not errors, "%d errors\n" % len(errors) + "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# The scrub calls at bit_locate's limits.

# configuration -> the limit it sits on, and one step past it
LIMITS = [
    (("cauchyrs", 30, 2, 8), "k = 30: all = 0x3FFFFFFF, k + m = 32", ("cauchyrs", 31, 2, 8)),
    (("cauchyrs", 12, 3, 32), "exactly 768 row words, w = 32", ("cauchyrs", 13, 3, 32)),
    (("cauchyrs", 6, 4, 32), "m = 4 at w = 32, 576 words", ("cauchyrs", 9, 4, 32)),
    (("liberation", 24, 2, 31), "744 words", ("liberation", 25, 2, 31)),
    (("liberation", 13, 2, 13), "the widest liberation code with kernels of its own", None),
]
PAST_W = ("cauchyrs", 6, 4, 33)  # past w = 32: no such code


def _lid(row):
    return "%s-%d-%d-%d" % row[0]


def _limit_case(le, oracle, cfg):
    cls, k, m, w = cfg
    return H.edge_case(le, oracle, cfg, T.sizes(cls, k, w)[0], n=k + m + 2)


def _heal_view(case, words):
    """(the words as run_heal must read them, the object it leaves out).
    run_heal expects an object whose word is LEOEC_LOCATE_MANY to stay as it
    was damaged.  At k + m = 32 (cauchyrs(30,2,8) here) bit 31 is both the id
    of the last coding block and LEOEC_LOCATE_MANY: from the word alone a
    caller cannot tell "no single block explains it" from "block 31", and
    include/leoec.h settles it as block 31 for leoec_heal_dev.  So for this
    one configuration the heal expectation follows the header's reading, it
    is not independent of it: object 31 (block 31 damaged) must come back
    healed, and run_heal is told a plain block word for it; the two-block
    object, whose word may be that same value, is left out of the heal
    comparison, as it is for every m = 2 code whose model word names a third
    block.  Verify and both locates compare every object at every
    configuration."""
    k, m = case.k, case.m
    words = list(words)
    two = case.n - 1
    skip = None if (words[two] == S.MANY and k + m < 32) else two
    if k + m == 32:
        assert words[31] == S.MANY == 1 << 31
        words[31] = 1 << 30  # (read only as "not LEOEC_LOCATE_MANY")
    return words, skip


def test_limits_served_and_one_step_past(le):
    cid = le._lib.CODING_IDS
    for cfg, _, past in LIMITS:
        cls, k, m, w = cfg
        assert W.served(*cfg), cfg
        assert le.lib.leoec_check_params(cid[cls], k, m, w) == 0
        assert (m - 1) * k * w <= W.MAX_WORDS and k + m <= 32
        assert len([x for rows in le.device.locate_bitrows(cls, (k, m, w)) for blk in rows
                    for x in blk]) == (m - 1) * k * w
        if past is None:
            continue
        pcls, pk, pm, pw = past
        assert not W.served(*past), past
        assert le.lib.leoec_check_params(cid[pcls], pk, pm, pw) == 0, past
        assert le.lib.leoec_locate_bitrows(cid[pcls], pk, pm, pw, None, 0) == E_UNSUPPORTED, past
        assert le.lib.leoec_locate_ws_dev_workspace(cid[pcls], pk, pm, pw, 4000, 1, None) == E_UNSUPPORTED
        assert le.lib.leoec_locate_ws_dev(cid[pcls], pk, pm, pw, None, 0, 4000, 1, None, 0, None,
                                          None, 0, None) == E_UNSUPPORTED, past
    assert (12 * 2 * 32, 6 * 3 * 32, 24 * 31, 13 * 13) == (768, 576, 744, 169)
    assert le.lib.leoec_check_params(cid[PAST_W[0]], *PAST_W[1:]) == E_UNSUPPORTED
    assert le.lib.leoec_locate_bitrows(cid[PAST_W[0]], *PAST_W[1:], None, 0) == E_UNSUPPORTED


@pytest.mark.parametrize("row", LIMITS, ids=_lid)
def test_limits_position_batch_against_oracle_and_model(le, oracle, row):
    """No GPU: the damage lies inside valid bytes, the oracle's re-encoding
    gives the by-construction flags and locate_ws_helpers.model_words the
    by-construction words."""
    case = _limit_case(le, oracle, row[0])
    k, m = case.k, case.m
    dmg, verify, locate = S.position_batch(case)
    assert len({(wh, o, p) for wh, o, p, _ in dmg}) == len(dmg)
    assert all(len(S.block_hits(case, b)) == S.HITS for b in range(k + m))
    S.damaged_objects(case, dmg)  # asserts every position inside valid bytes
    assert verify == [(1 << m) - 1] * k + [1 << i for i in range(m)] + [0, (1 << m) - 1]
    assert locate[:-1] == [1 << b for b in range(k + m)] + [0]
    assert S.oracle_flags(oracle, case, dmg) == verify, case.ident()
    want = S.two_block_word(oracle, le, case, dmg, locate)
    assert W.model_words(oracle, le, case, dmg) == want, case.ident()


@pytest.mark.gpu
@pytest.mark.parametrize("row", LIMITS, ids=_lid)
def test_scrub_at_locate_ws_limits(gpu, le, oracle, row):
    """verify, locate_ws, heal from the located words, locate_ws again."""
    case = _limit_case(le, oracle, row[0])
    dmg, verify, locate = S.position_batch(case)
    work, par = L.damaged_arenas(gpu, case, dmg)
    errors = S.check_verify(gpu, le, case, work, par, verify)
    want = S.two_block_word(oracle, le, case, dmg, locate)
    lost, errs = S.check_locate(gpu, le, case, work, par, want)
    errors += errs
    if not errs:  # heal takes the words as they are: not with wrong ones
        words, skip = _heal_view(case, want)
        errors += S.run_heal(gpu, le, case, work, par, lost, words, skip)
        again = [0] * (case.n - 1) + [want[-1]]
        errors += S.check_locate(gpu, le, case, work, par, again, skip)[1]
    assert not errors, "\n".join(errors[:20])


# ---------------------------------------------------------------------------
# bit_heal_list over its runtime parameters (scrub_ws_instances_child.py).

def test_bit_heal_list_sweep_is_what_it_claims(le, oracle):
    """No GPU: the groups hold every cauchyrs w = 2..32, the ten liberation
    widths, the limits and k = 1, each configuration once, at most 16 a group;
    every one is served by leoec_scrub_ws_dev (locate_ws_helpers.served and
    k + m <= 31), accepted by the oracle, and of the stated geometry."""
    cfgs = BC.configs()
    assert len(cfgs) == len(set(cfgs)) == 45
    assert sorted(c for g in BC.GROUPS.values() for c in g) == sorted(cfgs)
    assert all(len(g) == 15 <= BC.MAX_TABLES for g in BC.GROUPS.values())
    assert BC.MAX_WORDS == W.MAX_WORDS
    assert sorted({w for cls, _, _, w in cfgs if cls == "cauchyrs"}) == list(range(2, 33))
    assert sorted({w for cls, _, _, w in cfgs if cls == "liberation"}) == list(BC.LIB_WS)
    assert all(c in cfgs for c in BC.LIMITS + BC.ONES)
    assert BC.LIMITS == [("cauchyrs", 27, 4, 8), ("cauchyrs", 29, 2, 8), ("cauchyrs", 12, 3, 32),
                         ("cauchyrs", 6, 4, 32), ("liberation", 24, 2, 31)]
    assert BC.ONES == [("cauchyrs", 1, 2, 8), ("liberation", 1, 2, 3)]
    # the sweep's m: 2, 3 and 4 all met below w = 17, 3 and 4 above
    sweep = [BC.cauchy_config(w) for w in range(2, 33)]
    assert {m for _, _, m, w in sweep if w <= 16} == {2, 3, 4}
    assert {m for _, _, m, w in sweep if w > 16} == {3, 4}
    # what the limits sit on
    assert (27 + 4, 29 + 2, 2 * 12 * 32, 3 * 6 * 32, 24 * 31) == (31, 31, 768, 576, 744)
    assert (29 + 3) // 4 == 8  # 29 survivor ids: all 8 id words of a record
    cid = le._lib.CODING_IDS
    for cfg in cfgs:
        cls, k, m, w = cfg
        assert W.served(*cfg) and k + m <= 31 and m >= 2, cfg
        assert cls == "liberation" or k + m <= 1 << w, cfg
        assert oracle.check_params(*cfg) == 0 and le.lib.leoec_check_params(cid[cls], k, m, w) == 0, cfg
        assert len(oracle.encode(cls, k, m, w, b"\x5a")) == k + m
        szs = BC.sizes(cfg)
        assert len(szs) == (2 if k >= 2 else 1)
        n = k + m + 2
        B = BC.PACKET * w
        assert le.layout(cls, (k, m, w), szs[0])[0] == B
        assert H.block_valids(k, B, szs[0]) == [B] * (k - 1) + [B - 1]
        # a whole 1 KiB tile and a 16-byte one
        assert BC.PACKET // 1024 == 1 and BC.PACKET % 1024 == 16
        assert le.device.scrub_ws_workspace(cls, (k, m, w), szs[0], n) == \
            16 + (4 * n + 15) // 16 * 16 + n * m * B
        if k >= 2:
            assert le.layout(cls, (k, m, w), szs[1])[0] == 16 * w  # packets of 16 bytes: one lane of 64
            assert H.block_valids(k, 16 * w, szs[1]) == [16 * w] * (k - 1) + [5]


@pytest.mark.parametrize("name", sorted(BC.GROUPS))
def test_bit_heal_list_sweep_against_oracle_and_model(le, oracle, name):
    """No GPU: at both sizes of every configuration the whole-block damage
    lies inside valid bytes, no object but the clean one expects 0, the
    oracle's re-encoding gives the by-construction flags and
    locate_ws_helpers.model_word the by-construction words."""
    for cfg, size in [(cfg, size) for cfg in BC.GROUPS[name] for size in BC.sizes(cfg)]:
        cls, k, m, w = cfg
        case = H.EdgeCase(le, oracle, cfg, size, k + m + 1)
        blocks = S.whole_batch(case)
        words = S.whole_words(case, blocks)
        assert words == [1 << b for b in range(k + m)] + [0], cfg
        objs = S.whole_objects(case, blocks)
        assert sorted(objs) == list(range(k + m))
        flags = [(1 << m) - 1] * k + [1 << i for i in range(m)] + [0]
        assert S.flags_of(oracle, case, objs) == flags, cfg
        model = S.words_of(oracle, le, case, objs)
        assert [model[o] for o in range(case.n)] == words, cfg


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bit_heal_list_sweep_in_own_processes(gpu, tmp_path):
    """bit_heal_list at every configuration of the sweep, one group of at most
    16 per fresh process (the block table cache's bound); the first child that
    fails or dies ends the test and nothing is started after it.  The child's
    output goes to a log in the test's temporary directory; a failure shows
    its tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    for name in sorted(BC.GROUPS):
        log = str(tmp_path / f"bit_heal_list_{name}.log")
        cmd = [sys.executable, "-u", os.path.abspath(BC.__file__), name]
        with open(log, "w") as fh:
            rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                                 timeout=90)
        with open(log) as fh:
            text = fh.read()
        assert rc == 0, f"bit_heal_list sweep, group {name}, failed (rc {rc}), {log}:\n{text[-4000:]}"
        assert f"group {name}: {len(BC.GROUPS[name])} configurations scrubbed" in text, text[-4000:]
        lines = sum(len(BC.sizes(cfg)) for cfg in BC.GROUPS[name])
        assert text.count(" 0 errors") == lines, text[-4000:]
