"""Device-resident batches whose rows lie more than 4 GiB apart.

Every leoec_*_dev entry point takes 64-bit row strides and computes its
addresses as `base + o * stride`; some kernels form a raw buffer resource from
that address, others add a 32-bit lane offset to it.  Here every call runs on
three objects whose rows lie wide_helpers.STRIDE = 2^32 + 48 bytes apart, so
the row offsets 0, STRIDE and 2 STRIDE cross 2^32 and 2^33 and a stride kept
in 32 bits becomes 48.  The rows are regions of one device allocation (rows 0
and 1 whole and the used part of row 2, about 8.6 GB, filled on the device
once per module and never copied to the host): the objects at byte 0 of every
row, the parity, and for repair every block and every output each at its own
offset, all with the row stride STRIDE, at least 64 KiB of fill between them.
An address truncated to 32 bits puts row o's access `o * 48` bytes past the
same region of row 0, inside the allocation: a wrong kernel shows as wrong
bytes, not as a memory fault.  After each call every region of every row,
widened by 4 KiB on each side, is compared on the device byte for byte, and
every small buffer whole (wide_helpers.execute).

One object size per family, k B - 17 (a ragged last block that is no multiple
of 16, several whole tiles and a partial one), the oracle's blocks as every
expectation.  Which family reaches which kernel (test_device_edges.py's table
for encode, decode and repair):

  vandrs(10,4,8), (4,2,8), (7,3,8),  gf8_apply<K,R> (256 lanes; 64 lanes at bs 164,992);
  isars(10,4,8), vandrs bs 164,992     verify: gf8_check; locate: gf8_locate; heal: gf8_heal;
                                       scrub: gf8_locate, gf8_heal_list
  vandrs(20,4,8), vandrs(6,5,8)      gf8_apply, accumulating (k > 16) and in two row groups
                                       (m > 4); verify: encode + verify_compare; heal: gf8_apply
                                       per run of objects (the host's o0 * stride)
  cauchyrs(10,4,8), (6,3,4),         gfbit_apply<W,R>; verify: encode + verify_compare;
  (5,2,11)                             locate_ws: encode + bit_locate; scrub_ws: bit_heal_list
  liberation(4,2,7)                  lib_apply<7>, libb_dec_apply<7>; verify, locate_ws and
                                       scrub_ws as cauchyrs
  liberation(10,2,11)                libb_apply<11>, libb_dec_apply<11>; the same
  vandrs(10,4,16), vandrs(6,3,32)    gfs_apply<16|32,R>; verify: encode + verify_compare
  cauchyrs(5,3,17)                   bit_apply; verify, locate_ws and scrub_ws as cauchyrs

The two-pass calls (verify, locate_ws, scrub_ws) run once with the query's
workspace and once with room for one object, so that the chunk loop's
host-side `o0 * stride` advance runs as well.  heal, scrub and scrub_ws keep
per-process table caches and run in a fresh child process
(wide_strides_child.py), which asserts that the table path ran.

Not reached: gfbk_apply (launch_gfbk_t, cauchyrs(10,4,8) launches of 4 GB of
algorithmic bytes and more: with 3 objects that means blocks of about 95 MB,
which the oracle cannot encode in a few seconds; its row arithmetic is reached
up to 3.94 GiB by test_gpu_parity.py::test_cauchy_64MiB_objects_gfbk), and
workspace offsets past 4 GiB (the workspaces here are small)."""
import json
import os
import subprocess
import sys
import time

import pytest

import gpu_helpers as H
import scrub_dev_helpers as D
import verify_helpers as V
import wide_helpers as Wd
import wide_strides_child as C

E_UNSUPPORTED = -14  # LEOEC_E_UNSUPPORTED

_ids = Wd.family_id
_ran = {}       # case id -> seconds, of this module's in-process GPU cases
_arena = []     # the module's device allocation, while it is held
_times = {}     # test -> seconds


@pytest.fixture(scope="module")
def arena(gpu, le):
    """The module's one device allocation, filled once, released at teardown
    (and before the child process starts: `release`)."""
    def get():
        if not _arena:
            gpu.cuda.reset_peak_memory_stats()
            _arena.append(Wd.Arena(gpu, Wd.arena_used(le)))
        return _arena[0]
    yield get
    _release()


def _release():
    while _arena:
        _arena.pop().release()


def _status(call):
    from leo_erasure_amd._lib import LeoecError
    try:
        return 0, call()
    except LeoecError as e:
        return e.code, None


@pytest.mark.parametrize("family", Wd.FAMILIES, ids=_ids)
def test_wide_case_table(le, family):
    """The case table (no GPU): the stride and every offset a multiple of 16,
    the stride above 2^32, every widened region inside its row and apart from
    the next by 64 KiB of fill, truncated addresses inside the widened region
    of row 0, the allocation under its cap, the size as ragged as claimed, and
    the calls that serve the family as the library's own statuses say."""
    cls, k, m, w, B = family
    params = (k, m, w)
    S, lay, size = Wd.STRIDE, Wd.layout(le, family), Wd.size_of(family)
    assert S % 16 == 0 and S % 4096 and S > 2**32 and S % 2**32 == 48
    assert [o * S >= 2**32 for o in range(Wd.NOBJ)] == [False, True, True] and 2 * S >= 2**33
    assert family in H.EDGE_FAMILIES or family in Wd.FAMILIES[-2:]
    assert len(Wd.FAMILIES) == len(H.EDGE_FAMILIES) + 2 == 15
    spans = sorted(lay.regions.values())
    assert len(spans) == 2 + (k + m) + m and spans[0] == (0, lay.objs_cols) and lay.objs_cols >= size
    assert all(off % 16 == 0 for off, _ in spans)
    assert all(off % 4096 for off, _ in spans[1:])
    for (off, length), (nxt, _) in zip(spans, spans[1:]):
        assert nxt - (off + length) >= Wd.GAP          # neither they nor their widened forms overlap
        assert nxt - Wd.PAD > off + length + Wd.PAD
    for name in lay.regions:
        lo, hi = lay.widened(name)
        assert 0 <= lo and hi <= lay.used <= Wd.arena_used(le) < S
        assert hi - lo == lay.regions[name][1] + (Wd.PAD if name == "objs" else 2 * Wd.PAD)
    for _, trunc in Wd.truncations():
        assert [trunc(o) for o in range(Wd.NOBJ)] == [0, 48, 96] and trunc(Wd.NOBJ - 1) < Wd.PAD
    assert Wd.arena_bytes(le) == 2 * S + Wd.arena_used(le) <= Wd.CAP
    # the size: block size B, every block but the last whole, the last one 17 bytes short
    assert lay.bs == B == le.layout(cls, params, size)[0]
    valid = H.block_valids(k, lay.bs, size)
    assert valid[:-1] == [B] * (k - 1) and valid[-1] == B - 17 and valid[-1] % 16 == 15
    tile = 4096 if V.packet_tile(cls, w) is None else V.packet_tile(cls, w) * w
    assert B > 2 * tile and B % tile, "several whole tiles and a partial one"
    # the calls, against the library's statuses (none of these needs a device)
    dev, kinds = le.device, {kind for kind, _ in Wd.calls(family)}
    assert {"encode", "decode", "repair", "verify"} <= kinds
    assert Wd.erasures(family) == [list(range(k - m, k)), sorted(([0, k - 1] + list(range(k, k + m)))[:m])]
    rc, need = _status(lambda: dev.verify_workspace(cls, params, size, Wd.NOBJ))
    assert rc == 0 and need == (0 if ("verify", "fused") in Wd.calls(family) else Wd.NOBJ * m * B)
    rc, _ = _status(lambda: dev.heal_rows(cls, params, 1, coef=False))
    assert (rc == 0) == ("heal" in kinds) and "heal" in kinds
    rc, _ = _status(lambda: dev.locate_rows(cls, params))
    assert rc == (0 if "locate" in kinds else E_UNSUPPORTED)
    assert ("scrub" in kinds) == ("locate" in kinds)
    rc, need = _status(lambda: dev.scrub_workspace(cls, params, size, Wd.NOBJ))
    assert (rc, need) == ((0, D.head(Wd.NOBJ)) if "scrub" in kinds else (E_UNSUPPORTED, None))
    rc, _ = _status(lambda: dev.locate_bitrows(cls, params))
    assert rc == (0 if "locate_ws" in kinds else E_UNSUPPORTED)
    rc, need = _status(lambda: dev.locate_ws_workspace(cls, params, size, Wd.NOBJ))
    if "locate" in kinds:
        assert (rc, need) == (0, 0)
    else:
        assert (rc, need) == ((0, Wd.NOBJ * m * B) if "locate_ws" in kinds else (E_UNSUPPORTED, None))
    rc, need = _status(lambda: dev.scrub_ws_workspace(cls, params, size, Wd.NOBJ))
    if "scrub" in kinds:
        assert (rc, need) == (0, D.head(Wd.NOBJ))
    elif "scrub_ws" in kinds:
        assert (rc, need) == (0, D.head(Wd.NOBJ) + Wd.NOBJ * m * B) and "locate_ws" in kinds
    else:
        assert rc == E_UNSUPPORTED and "locate_ws" not in kinds


def test_wide_case_counts():
    """The table as a whole: 15 families, every call kind present, the ids
    unique, the child's share what wide_strides_child.py runs."""
    every = Wd.case_ids(("encode", "decode", "repair", "verify", "locate", "locate_ws") + Wd.CHILD_KINDS)
    assert len(set(every)) == len(every)
    count = lambda kind: sum(1 for c in every if f":{kind}:" in c)  # noqa: E731
    assert [count(kd) for kd in ("encode", "decode", "repair", "heal")] == [15, 30, 30, 15]
    assert count("verify") == 5 + 2 * 10 and count("locate") == 5 == count("scrub")
    assert count("locate_ws") == 12 == count("scrub_ws")


# one family per kernel family: gf8, gfbit, lib, libb, gfs, bit
SIM_FAMILIES = [("vandrs", 4, 2, 8, 8704), ("cauchyrs", 6, 3, 4, 4352 * 4), ("liberation", 4, 2, 7, 2176 * 7),
                ("liberation", 10, 2, 11, 2176 * 11), ("vandrs", 10, 4, 16, 8704),
                ("cauchyrs", 5, 3, 17, 8704 * 17)]


@pytest.mark.parametrize("family", SIM_FAMILIES, ids=_ids)
def test_wide_compare_can_fail(le, oracle, family):
    """The comparison can fail (no GPU; the stand-in for a deliberately broken
    kernel, which is never built): for each call kind the compare functions
    are given what the expectation itself holds, and find nothing; then what a
    kernel leaves that kept a row offset or a stride in 32 bits
    (wide_helpers.simulate), and report an error that names row 1 or row 2."""
    assert family in Wd.FAMILIES
    seen = set()
    for kind, var in Wd.calls(family):
        if kind in seen:
            continue
        seen.add(kind)
        p = Wd.plan(le, oracle, family, kind, var)
        assert Wd.compare(p.lay, p.want, p.want) == [] and Wd.compare_words(p.words_want, p.words_want) == []
        for name, trunc in Wd.truncations():
            got, words = Wd.simulate(p, trunc)
            errors = Wd.compare(p.lay, got, p.want) + Wd.compare_words(words, p.words_want)
            assert any("row 1" in e or "row 2" in e for e in errors), (p.ident(), name, errors)
            if p.outputs:  # the regions alone tell
                assert any("row 1 region" in e or "row 2 region" in e
                           for e in Wd.compare(p.lay, got, p.want)), (p.ident(), name)
            else:          # a read-only call: the words tell
                assert any("row 1" in e or "row 2" in e
                           for e in Wd.compare_words(words, p.words_want)), (p.ident(), name, words)
    assert {"encode", "decode", "repair", "verify", "heal"} <= seen
    assert ("locate" in seen and "scrub" in seen) or ("locate_ws" in seen and "scrub_ws" in seen) \
        or family[3] in (16, 32)


def _run(gpu, le, oracle, arena, family, kinds):
    t0 = time.monotonic()
    errors, todo = [], [(kind, var) for kind, var in Wd.calls(family) if kind in kinds]
    assert todo
    for kind, var in todo:
        t1 = time.monotonic()
        p = Wd.plan(le, oracle, family, kind, var)
        errors += Wd.execute(gpu, le, arena(), p)
        _ran[p.ident()] = time.monotonic() - t1
    _times[f"{'+'.join(kinds)} {_ids(family)}"] = time.monotonic() - t0
    assert not errors, "\n".join(errors[:12])


@pytest.mark.gpu
@pytest.mark.parametrize("family", Wd.FAMILIES, ids=_ids)
def test_wide_encode(gpu, le, oracle, arena, family):
    _run(gpu, le, oracle, arena, family, ("encode",))


@pytest.mark.gpu
@pytest.mark.parametrize("family", Wd.FAMILIES, ids=_ids)
def test_wide_decode(gpu, le, oracle, arena, family):
    """The last m data blocks erased; the first and the last data block plus
    coding blocks.  The erased blocks are poisoned first."""
    _run(gpu, le, oracle, arena, family, ("decode",))


@pytest.mark.gpu
@pytest.mark.parametrize("family", Wd.FAMILIES, ids=_ids)
def test_wide_repair(gpu, le, oracle, arena, family):
    """Every block and every output a region of its own in the rows."""
    _run(gpu, le, oracle, arena, family, ("repair",))


@pytest.mark.gpu
@pytest.mark.parametrize("family", Wd.FAMILIES, ids=_ids)
def test_wide_verify(gpu, le, oracle, arena, family):
    """Object 0 clean, a coding block of object 1 and a data block of object 2
    damaged; two-pass families with the query's workspace and with one
    object's."""
    _run(gpu, le, oracle, arena, family, ("verify",))


@pytest.mark.gpu
@pytest.mark.parametrize("family", [f for f in Wd.FAMILIES if Wd.located(f) or Wd.located_ws(f)], ids=_ids)
def test_wide_locate(gpu, le, oracle, arena, family):
    """locate, or locate_ws for its class (b) with the query's workspace and
    with one object's; different blocks damaged in objects 1 and 2."""
    _run(gpu, le, oracle, arena, family, ("locate", "locate_ws"))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_heal_and_scrub_in_own_process(gpu, le, arena, tmp_path):
    """The heal, scrub and scrub_ws cases in one fresh child process with
    fresh table caches (wide_strides_child.py), which holds an allocation of
    its own; this process releases its own first.  The child reports per case
    as JSON; every case of the table must have run, with no error and, for
    scrub and scrub_ws, on the kernel path."""
    _release()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    log = str(tmp_path / "wide_strides_child.log")
    t0 = time.monotonic()
    with open(log, "w") as fh:
        rc = subprocess.call([sys.executable, "-u", os.path.abspath(C.__file__)], cwd=root, env=env,
                             stdout=fh, stderr=subprocess.STDOUT, timeout=240)
    _times["child process"] = time.monotonic() - t0
    with open(log) as fh:
        text = fh.read()
    assert rc == 0, f"wide-stride child failed (rc {rc}), {log}:\n{text[-4000:]}"
    lines = [json.loads(x) for x in text.splitlines() if x.startswith("{")]
    cases, last = lines[:-1], lines[-1]
    errors = [e for c in cases for e in c["errors"]]
    assert not errors, "\n".join(errors[:12])
    assert sorted(c["case"] for c in cases) == Wd.case_ids(Wd.CHILD_KINDS)
    assert last["done"] == len(cases) and last["pattern_tables"] == 4 and last["block_tables"] == 6
    assert all(c["path"] == "list" for c in cases if ":heal:" not in c["case"])
    assert last["peak_bytes"] <= Wd.CAP
    print(f"child: {len(cases)} cases, peak device memory {last['peak_bytes']} B, slowest case "
          f"{max(c['seconds'] for c in cases)} s, process {_times['child process']:.1f} s")


@pytest.mark.gpu
def test_wide_every_case_ran(gpu, le):
    """Every family x call of the table ran in this module's process (the
    child's share is asserted by its own test), under the allocation's cap."""
    assert sorted(_ran) == Wd.case_ids(("encode", "decode", "repair", "verify", "locate", "locate_ws"))
    peak = gpu.cuda.max_memory_allocated()
    assert peak <= Wd.CAP
    slow = max(_times, key=_times.get)
    print(f"in-process: {len(_ran)} cases, peak device memory {peak} B, slowest test {slow} "
          f"{_times[slow]:.2f} s, all tests {sum(_times.values()):.1f} s")
