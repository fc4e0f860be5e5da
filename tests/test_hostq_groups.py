"""Group-wise completion in the batching queue (hostq.cpp,
Knobs::hostq_done_groups): a large batch's output comes back in up to G
copies, one per contiguous group of its jobs, and a group's callers are woken
when their copy has landed.

32 threads call the C ABI at once; each makes 8 encodes, then 8 decodes with
data blocks {0,1,2,3} erased and 4 repairs of {0,5,10,13}, vandrs RS(10,4,8),
every object of its own random bytes at a size drawn from {4,096, 65,537,
262,144, 1,048,576} B: batches then hold several runs of different maps and
group boundaries fall inside runs.  Every caller's output buffer is filled
with 0xA5 before each call and must equal the oracle's bytes afterwards (every
thread's objects differ, so another caller's output in it is a mismatch).

The product library runs its shipped G in this process; the measurement
library runs G = 1, 2, 4 and 8 (LEOEC_HOSTQ_DONE_GROUPS), every call through
the queue, each in a child process (this file is its script).  With
LEOEC_HOSTQ_FAIL_BS set to one size's block size exactly that size's calls
fail with LEOEC_E_HIP and every other call of the same batches is bit-exact.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

THREADS = 32
SIZES = [4096, 65537, 262144, 1048576]
K, M, W = 10, 4, 8
ERASED = [0, 1, 2, 3]
REPAIR = [0, 5, 10, 13]
POISON = 0xA5
FAIL_SIZE = 65537


def block_size(size):
    return (-(-size // (K * W)) + 15) // 16 * 16 * W


def plan(t):
    """Thread t's sizes: 8 encodes, 8 decodes, 4 repairs."""
    rng = np.random.Generator(np.random.PCG64(1000 + t))
    return [SIZES[i] for i in rng.integers(0, len(SIZES), 20)]


_objects = {}


def objects(le, oracle):
    """{(thread, size): (data, blocks)}: every thread's own object of every
    size it uses, the oracle's blocks computed once."""
    if not _objects:
        for t in range(THREADS):
            for size in sorted(set(plan(t))):
                rng = np.random.Generator(np.random.PCG64(t * 7919 + size))
                data = rng.integers(0, 256, size, dtype=np.uint8)
                ref = oracle.encode("vandrs", K, M, W, data.tobytes())
                _objects[(t, size)] = (data, [np.frombuffer(b, dtype=np.uint8).copy() for b in ref],
                                       le.layout("vandrs", (K, M, W), size)[1])
    return _objects


def caller(le, objs, t, fail_size):
    """Thread t's 20 calls; (errors, calls that failed as injected)."""
    L, cid, E_HIP = le.lib, le._lib.CODING_IDS["vandrs"], le._lib.E_HIP
    errs, injected = [], 0

    def judge(what, size, rc, equal):
        nonlocal injected
        if fail_size is not None and size == fail_size:
            if rc == E_HIP:
                injected += 1
            else:
                errs.append(f"thread {t}: {what} size {size}: expected the injected failure, rc {rc}")
        elif rc or not equal:
            errs.append(f"thread {t}: {what} size {size}: rc {rc}, bit-exact {equal}")

    for i, size in enumerate(plan(t)):
        data, blocks, filled = objs[(t, size)]  # (encode writes blocks filled .. k + m - 1)
        bs = len(blocks[0])
        assert bs == block_size(size)
        if i < 8:
            out = np.full((K + M - filled) * bs, POISON, dtype=np.uint8)
            rc = L.leoec_encode(cid, K, M, W, data.ctypes.data, size, out.ctypes.data, out.size)
            judge("encode", size, rc,
                  out.tobytes() == b"".join(b.tobytes() for b in blocks[filled:]))
        elif i < 16:
            ids = [b for b in range(K + M) if b not in ERASED]
            ptrs = (ctypes.c_void_p * len(ids))(*[blocks[b].ctypes.data for b in ids])
            idv = (ctypes.c_int * len(ids))(*ids)
            out = np.full(size, POISON, dtype=np.uint8)
            rc = L.leoec_decode(cid, K, M, W, ptrs, idv, len(ids), bs, size, out.ctypes.data)
            judge("decode", size, rc, bool(np.array_equal(out, data)))
        else:
            ids = [b for b in range(K + M) if b not in REPAIR]
            ptrs = (ctypes.c_void_p * len(ids))(*[blocks[b].ctypes.data for b in ids])
            idv = (ctypes.c_int * len(ids))(*ids)
            rep = (ctypes.c_int * len(REPAIR))(*REPAIR)
            out = np.full(len(REPAIR) * bs, POISON, dtype=np.uint8)
            rc = L.leoec_repair(cid, K, M, W, ptrs, idv, len(ids), bs, rep, len(REPAIR),
                                out.ctypes.data)
            judge("repair", size, rc,
                  out.tobytes() == b"".join(blocks[b].tobytes() for b in REPAIR))
    return errs, injected


def run_callers(le, oracle, fail_size=None):
    import concurrent.futures as cf
    objs = objects(le, oracle)
    with cf.ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(lambda t: caller(le, objs, t, fail_size), range(THREADS)))
    return [e for errs, _ in res for e in errs], sum(n for _, n in res)


def test_plan_mixes_sizes():
    """(no GPU) every size is used, by many threads, in every kind of call."""
    plans = [plan(t) for t in range(THREADS)]
    for lo, hi in ((0, 8), (8, 16), (16, 20)):
        assert {s for p in plans for s in p[lo:hi]} == set(SIZES)
    assert block_size(1048576) == 104960 and block_size(FAIL_SIZE) == 6656
    assert len({block_size(s) for s in SIZES}) == len(SIZES)


@pytest.mark.gpu
def test_shipped_groups(gpu, le, oracle):
    errs, _ = run_callers(le, oracle)
    assert not errs, "\n".join(errs[:10])


def _run_child(extra_env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(os.path.join(root, "leo_erasure_amd", "libleoec_measure.so")):
        pytest.fail("measurement build absent (make -C leo_erasure_amd/csrc measure)")
    env = dict(os.environ, LEOEC_LIBRARY="measure", LIBC_FATAL_STDERR_="1",
               LEOEC_HOSTQ_DIRECT="0", LEOEC_HOSTQ_DIRECT_MAP="0", **extra_env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("groups", ["1", "2", "4", "8"])
def test_groups_measurement_build(gpu, groups):
    out = _run_child({"LEOEC_HOSTQ_DONE_GROUPS": groups})
    assert not out["errors"], "\n".join(out["errors"][:10])
    # every call went through the queue, several jobs per batch, several maps per batch
    assert out["jobs"] == THREADS * 20 and out["batches"] < out["jobs"], out
    assert out["launches"] > out["batches"], out


@pytest.mark.gpu
@pytest.mark.parametrize("groups", ["1", "4"])
def test_one_size_fails_alone(gpu, groups):
    out = _run_child({"LEOEC_HOSTQ_DONE_GROUPS": groups,
                      "LEOEC_HOSTQ_FAIL_BS": str(block_size(FAIL_SIZE))})
    assert not out["errors"], "\n".join(out["errors"][:10])
    want = sum(1 for t in range(THREADS) for s in plan(t) if s == FAIL_SIZE)
    assert out["injected"] == want > 0, out


def _child():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import leo_erasure_amd as le
    from leo_erasure_amd import _lib
    from oracle import oracle as O
    assert _lib.is_measure_build(), "the child runs the measurement library"
    assert le.gf_init() == "ok"
    fail = FAIL_SIZE if os.environ.get("LEOEC_HOSTQ_FAIL_BS") else None
    stats = _lib._current.leoec_measure_hostq_stats
    buf = (ctypes.c_double * 14)()
    objects(le, O)
    stats(buf)
    errs, injected = run_callers(le, O, fail)
    stats(buf)
    print(json.dumps({"errors": errs[:20], "injected": injected, "batches": buf[0], "jobs": buf[1],
                      "launches": buf[2]}))
    return 0


if __name__ == "__main__":
    sys.exit(_child())
