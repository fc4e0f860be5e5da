"""Every compiled instance of the fused GF(2^8) family, run once with an
expectation from the oracle, in the product library.

gf8_check<K,R>, gf8_locate<K,R>, gf8_heal<K> and gf8_apply<K,R,acc> are
compiled per input count K = 1..16 (R = 1..4); what differs between the
instances (the id words and the record stride of gf8_heal, gf8_locate's loop
over the data blocks with its per-trip table loads, the register allocation
of the widest ones) is what one of them can get wrong alone.  The other device
tests reach K = 4, 7, 10 and 16.  Here: vandrs and isars, w = 8, k = 1..16,
m = 1..4, all 128 configurations, at two sizes:

  4224 k - 3      bs 4,224: one full 256-lane tile and a 128-byte edge tile,
                  the last block 3 bytes short (`full` true for tile 0 only)
  128 (k-1) + 5   bs 128, the last block 5 bytes

Per configuration, on the edge harness of gpu_helpers:
  verify   of scrub_helpers' position batch: gf8_check<k,m>, every flag bit
           set alone once and every data block setting all;
  locate   of the same batch, m >= 2: gf8_locate<k,m>, every block named once
           (m = 1: LEOEC_E_UNSUPPORTED);
  encode   gf8_apply<k,m,false>;
  decode   of the last r and of the first r data blocks, r = 1..min(k,m):
           gf8_apply<k,r,false> with decoding coefficients.
k = 17..32 runs the accumulating instances: the second input group of an
encode or a decode of m blocks is gf8_apply<k-16,m,true>.

gf8_heal<K> keeps at most 16 pattern tables per process (heal.hip), after
which a configuration silently takes the generic path; a sweep in this process
would test gf8_heal for a handful of K that depends on the order of the tests.
tests/gf8_heal_instances_child.py heals exactly 16 configurations, one per K,
in a process of its own; test_gf8_heal_every_k_in_own_process starts it twice
(test_heal_cpu.py::test_heal_rows_every_fused_configuration pins the table
contents of the configurations neither child launches).  The 64-lane form
stays with the families that cover it: the instance is the same.

gf8_heal_list<K> (leoec_scrub_dev's rebuild) depends on the same 16 tables:
tests/scrub_instances_child.py scrubs one configuration per K, m = 2..4, in a
process of its own, with scrub_helpers' whole-block batch and its position
batch, and reads from the workspace that the kernel path ran."""
import os
import subprocess
import sys

import pytest

import gf8_heal_instances_child as C
import scrub_instances_child as SC
import gpu_helpers as H
import locate_helpers as L
import scrub_helpers as S

CLASSES = ("vandrs", "isars")
E_UNSUPPORTED = -14


sizes = C.sizes  # [4224 k - 3, 128 (k-1) + 5]


def _cases(le, oracle, cls, k, m):
    for size in sizes(k):
        yield H.edge_case(le, oracle, (cls, k, m, 8), size, n=k + m + 2)


def erasures(k, m):
    """The last r data blocks, then the first r, r = 1..min(k, m)."""
    out = []
    for r in range(1, min(k, m) + 1):
        for s in (list(range(k - r, k)), list(range(r))):
            if s not in out:
                out.append(s)
    return out


CONFIGS = [(cls, k) for cls in CLASSES for k in range(1, 17)]
WIDE = [(cls, k) for cls in CLASSES for k in range(17, 33)]


def _id(c):
    return "%s-k%d" % c


def test_instance_table(le, oracle):
    """No GPU: the oracle and the library accept all 128 + 128 configurations,
    the library serves the fused check for k <= 16, the sizes have the block
    geometry the module claims, and the erasure sets reach every r."""
    for cls, k in CONFIGS + WIDE:
        for m in range(1, 5):
            assert oracle.check_params(cls, k, m, 8) == 0, (cls, k, m)
            assert le.lib.leoec_check_params(le._lib.CODING_IDS[cls], k, m, 8) == 0, (cls, k, m)
            if k <= 16:
                assert le.device.verify_workspace(cls, (k, m, 8), sizes(k)[0], 4) == 0
                assert L.served(cls, k, m, 8) == (m >= 2)
                assert sorted({len(s) for s in erasures(k, m)}) == list(range(1, min(k, m) + 1))
        big, small = sizes(k)
        assert le.layout(cls, (k, 4, 8), big)[0] == 4224
        assert H.block_valids(k, 4224, big)[-1] == 4221
        if k <= 16:
            assert le.layout(cls, (k, 4, 8), small)[0] == 128
            assert H.block_valids(k, 128, small)[-1] == 5
    # one full 256-lane tile, then an edge tile
    assert 4224 // 4096 == 1 and 4224 % 4096 == 128


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_position_batches_against_oracle_and_model(le, oracle, cfg):
    """No GPU: for every case of test_gf8_instance the damage lies inside
    valid bytes, the oracle's re-encoding gives the by-construction flags and
    the host model the by-construction words."""
    cls, k = cfg
    for m in range(1, 5):
        for case in _cases(le, oracle, cls, k, m):
            dmg, verify, locate = S.position_batch(case)
            assert len({(wh, o, p) for wh, o, p, _ in dmg}) == len(dmg)
            assert all(len(S.block_hits(case, b)) == min(S.HITS, S.block_valid(case, b))
                       for b in range(k + m))
            assert verify == [(1 << m) - 1] * k + [1 << i for i in range(m)] + [0, (1 << m) - 1]
            assert S.oracle_flags(oracle, case, dmg) == verify, case.ident()
            if m == 1:
                continue
            assert locate[:-1] == [1 << b for b in range(k + m)] + [0]
            model = S.model_words(oracle, le, case, dmg)
            want = S.two_block_word(oracle, le, case, dmg, locate)
            assert [model[o] for o in range(case.n)] == want, case.ident()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_gf8_instance(gpu, le, oracle, cfg):
    """gf8_check<k,m>, gf8_locate<k,m>, gf8_apply<k,m,false> and
    gf8_apply<k,r,false>, m = 1..4, at both sizes."""
    cls, k = cfg
    errors = []
    for m in range(1, 5):
        for case in _cases(le, oracle, cls, k, m):
            dmg, verify, locate = S.position_batch(case)
            work, par = L.damaged_arenas(gpu, case, dmg)
            errors += S.check_verify(gpu, le, case, work, par, verify)
            if m == 1:
                try:
                    S.run_locate(gpu, le, case, work, par)
                    errors.append(f"locate {case.ident()}: m = 1 was served")
                except le.LeoecError as e:
                    if e.code != E_UNSUPPORTED:
                        errors.append(f"locate {case.ident()}: status {e.code}")
            else:
                want = S.two_block_word(oracle, le, case, dmg, locate)
                errors += S.check_locate(gpu, le, case, work, par, want)[1]
            err = H.check_encode(gpu, le, case)
            if err:
                errors.append(err)
            for erased in erasures(k, m):
                err = H.check_decode(gpu, le, case, erased)
                if err:
                    errors.append(err)
    assert not errors, "\n".join(errors[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", WIDE, ids=_id)
def test_gf8_accumulating_instance(gpu, le, oracle, cfg):
    """k = 17..32: encode (gf8_apply<16,m,false>, then <k-16,m,true>) and a
    decode of the last m data blocks (the same pair with decoding
    coefficients), 3 objects of 4224 k - 3 bytes."""
    cls, k = cfg
    errors = []
    for m in range(1, 5):
        case = H.edge_case(le, oracle, (cls, k, m, 8), sizes(k)[0], n=3)
        for err in (H.check_encode(gpu, le, case),
                    H.check_decode(gpu, le, case, list(range(k - m, k)))):
            if err:
                errors.append(err)
    assert not errors, "\n".join(errors[:20])


def test_heal_child_groups():
    """No GPU: each group of the heal child has one configuration per
    K = 1..16, both classes and every m; together they are 32 different ones."""
    for name in ("a", "b"):
        group = C.GROUPS[name]
        assert len(group) == 16 == C.MAX_TABLES
        assert sorted(k for _, k, _ in group) == list(range(1, 17))
        assert {cls for cls, _, _ in group} == set(CLASSES)
        assert {m for _, _, m in group} == {1, 2, 3, 4}
    for k in range(1, 17):
        assert ("vandrs" if k % 2 else "isars", k, 1 + (k - 1) % 4) in C.GROUPS["a"]
        assert ("isars" if k % 2 else "vandrs", k, 1 + (k + 1) % 4) in C.GROUPS["b"]
    assert len(set(C.GROUPS["a"]) | set(C.GROUPS["b"])) == 32
    for k, m in ((1, 1), (1, 3), (2, 4), (10, 4), (16, 4), (15, 3)):
        masks = C.masks_of(k, m)
        singles = k + m
        assert masks[:singles] == [1 << b for b in range(singles)]
        assert len(masks) == singles * m + 3
        assert all(a != b for a, b in zip(masks, masks[1:]))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_gf8_heal_every_k_in_own_process(gpu, tmp_path):
    """gf8_heal<K> for every K, 16 configurations per fresh process (the
    table cache's bound), group a and then group b; the first child that
    fails or dies ends the test and nothing is started after it.  The
    child's output goes to a log in the test's temporary directory; a failure
    shows its tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    for name in ("a", "b"):
        log = str(tmp_path / f"gf8_heal_{name}.log")
        cmd = [sys.executable, "-u", os.path.abspath(C.__file__), name]
        with open(log, "w") as fh:
            rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT,
                                 timeout=130)
        with open(log) as fh:
            tail = fh.read()[-4000:]
        assert rc == 0, f"heal instances, group {name}, failed (rc {rc}), {log}:\n{tail}"
        assert f"group {name}: 16 configurations healed" in tail, tail


def test_scrub_child_configurations(le):
    """No GPU: the scrub child has one configuration per K = 1..16, m cycling
    over 2..4 (scrub needs m >= 2), the classes alternating; every one is
    served; its sizes are this module's and have no empty data block."""
    assert len(SC.CONFIGS) == 16 == SC.MAX_TABLES == C.MAX_TABLES
    assert [k for _, k, _ in SC.CONFIGS] == list(range(1, 17))
    assert [m for _, _, m in SC.CONFIGS] == [2, 3, 4] * 5 + [2]
    assert [cls for cls, _, _ in SC.CONFIGS] == ["vandrs", "isars"] * 8
    for cls, k, m in SC.CONFIGS:
        assert L.served(cls, k, m, 8)
        assert le.device.scrub_workspace(cls, (k, m, 8), SC.sizes(k)[0], k + m + 2) == \
            16 + (4 * (k + m + 2) + 15) // 16 * 16
        assert SC.sizes(k) == sizes(k)
        for size, bs, last in zip(sizes(k), (4224, 128), (4221, 5)):
            assert le.layout(cls, (k, m, 8), size)[0] == bs
            assert H.block_valids(k, bs, size) == [bs] * (k - 1) + [last]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_gf8_heal_list_every_k_in_own_process(gpu, tmp_path):
    """gf8_heal_list<K> for every K, 16 configurations in one fresh process
    (the table cache's bound).  The child's output goes to a log in the test's
    temporary directory; a failure shows its tail."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LIBC_FATAL_STDERR_="1")
    env.pop("LEOEC_LIBRARY", None)
    log = str(tmp_path / "gf8_heal_list.log")
    cmd = [sys.executable, "-u", os.path.abspath(SC.__file__)]
    with open(log, "w") as fh:
        rc = subprocess.call(cmd, cwd=root, env=env, stdout=fh, stderr=subprocess.STDOUT, timeout=130)
    with open(log) as fh:
        text = fh.read()
    assert rc == 0, f"scrub instances failed (rc {rc}), {log}:\n{text[-4000:]}"
    assert "16 configurations scrubbed" in text, text[-4000:]
    assert text.count(" 0 errors") == 32, text[-4000:]  # one line per configuration and size
