"""gf8_apply's edge tiles (kernels_impl.hpp gf8_load / gf8_init_store /
gf8_store, the path of a tile that crosses a shard's valid length): loads
through a resource that ends at the valid length, the straddling chunk
cleared after the loads, whole chunks stored through a resource that ends at
the last whole chunk and the straddling lane's bytes stored one by one.

Device encode / decode / repair of vandrs (w = 8) against the CPU oracle on 8
objects, at the smallest shapes that reach each branch:

  1 B, 15 B            one chunk, straddled (nothing whole to store)
  k 8704 - 15          the last data block's valid length = 1 (mod 16): whole
                       tiles, then a tile with whole chunks and a straddling one
  k 2048 - 16          valid = 0 (mod 16) below a tile: no straddling lane, the
                       store resource ends inside the tile
  (k - 1) 128 k + 5    the last block holds 5 bytes: vmin < 16, every tile guarded
  1 MiB                bs 104,960, the last block 103,936: the last tile alone
  1 MiB + 1            the same with a straddling chunk

for (k, m) = (10, 4) and (4, 2), and k = 20 (two chained launches, the second
accumulating into the first's outputs: gf8_init_store's loads).  Decode erases
the sets that make the ragged last block an output with every survivor full
([6,7,8,9], [0,1,2,9] for k = 10).  Every object row, parity row and repair
row is followed by 4 KiB of 0xA5 (so is each tensor: its last row's), and
every byte of every tensor is compared afterwards: outputs equal to the
oracle's, guards and inputs untouched.

The product library runs its shipped tile widths in this process; the
measurement library runs the same cases with 64- and 256-lane tiles forced
(LEOEC_GF8_WG), each in a child process (this file is its script).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

GUARD = 4096
FILL = 0xA5
POISON = 0x5A
N = 8
CONFIGS = [(10, 4), (4, 2)]
CHAINED = (20, 4)


def sizes(k):
    return [1, 15, k * 8704 - 15, k * 2048 - 16, (k - 1) * 128 * k + 5, 1 << 20, (1 << 20) + 1]


def chained_sizes(k):
    return [1, k * 8704 - 15, (k - 1) * 128 * k + 5]


def erasures(k, m):
    return [list(range(k - m, k)), list(range(m - 1)) + [k - 1]]


def repairs(k, m):
    return [[0, 5, 10, 13]] if (k, m) == (10, 4) else [[0, k + m - 1]]


_cases = {}


def case(le, oracle, k, m, size):
    """Rows and the oracle's blocks of N objects, computed once per shape."""
    key = (k, m, size)
    if key not in _cases:
        bs, _ = le.layout("vandrs", (k, m, 8), size)
        rng = np.random.Generator(np.random.PCG64(size * 13 + k))
        data = rng.integers(0, 256, (N, size), dtype=np.uint8)
        blocks = np.empty((k + m, N, bs), dtype=np.uint8)
        for o in range(N):
            ref = oracle.encode("vandrs", k, m, 8, data[o].tobytes())
            for b in range(k + m):
                blocks[b, o] = np.frombuffer(ref[b], dtype=np.uint8)
        _cases[key] = (bs, data, blocks)
    return _cases[key]


def arena(gpu, payload):
    """[N, width + GUARD] device tensor: `payload` ([N, width]) then 0xA5."""
    host = np.full((N, (payload.shape[1] + 15) // 16 * 16 + GUARD), FILL, dtype=np.uint8)
    host[:, :payload.shape[1]] = payload
    return gpu.from_numpy(host).cuda()


def diff(gpu, got, want, what):
    if gpu.equal(got, want):
        return None
    ne = (got != want).nonzero()
    r, c = int(ne[0, 0]), int(ne[0, 1])
    return (f"{what}: {ne.shape[0]} bytes differ (rows of {got.shape[1]} B); first at row {r} byte {c}: "
            f"got 0x{int(got[r, c]):02X}, expected 0x{int(want[r, c]):02X}")


def run_shape(gpu, le, oracle, k, m, size):
    """Encode, the decodes and the repair of one shape; the list of errors."""
    p = (k, m, 8)
    bs, data, blocks = case(le, oracle, k, m, size)
    ctx = f"vandrs{p} size {size} bs {bs}"
    errs = []
    objs_snap = arena(gpu, data)
    parity = np.concatenate([blocks[k + i] for i in range(m)], axis=1)
    par_snap = arena(gpu, parity)

    objs = objs_snap.clone()
    par = arena(gpu, np.full((N, m * bs), FILL, dtype=np.uint8))
    le.device.encode("vandrs", p, objs, size, par)
    gpu.cuda.synchronize()
    errs += [diff(gpu, par, par_snap, f"encode {ctx}: parity"),
             diff(gpu, objs, objs_snap, f"encode {ctx}: objs")]

    for erased in erasures(k, m):
        objs, par = objs_snap.clone(), par_snap.clone()
        for e in erased:
            lo, hi = e * bs, min((e + 1) * bs, size)
            if lo < hi:
                objs[:, lo:hi] = POISON
        le.device.decode("vandrs", p, objs, size, par, erased)
        gpu.cuda.synchronize()
        errs += [diff(gpu, objs, objs_snap, f"decode {ctx} erased {erased}: objs"),
                 diff(gpu, par, par_snap, f"decode {ctx} erased {erased}: parity")]

    for lost in repairs(k, m):
        snaps = {b: arena(gpu, blocks[b]) for b in range(k + m) if b not in lost}
        avail = [snaps[b].clone() if b in snaps else None for b in range(k + m)]
        outs = [arena(gpu, np.full((N, bs), FILL, dtype=np.uint8)) for _ in lost]
        le.device.repair("vandrs", p, avail, bs, lost, outs, N)
        gpu.cuda.synchronize()
        for o, b in zip(outs, lost):
            errs.append(diff(gpu, o, arena(gpu, blocks[b]), f"repair {ctx} lost {lost}: block {b}"))
        for b, s in snaps.items():
            errs.append(diff(gpu, avail[b], s, f"repair {ctx} lost {lost}: input block {b}"))
    return [e for e in errs if e]


def all_shapes():
    return ([(k, m, s) for k, m in CONFIGS for s in sizes(k)] +
            [CHAINED + (s,) for s in chained_sizes(CHAINED[0])])


def test_shapes_reach_the_branches(le):
    """The table through the library's own layout (no GPU)."""
    for k, m in CONFIGS + [CHAINED]:
        v = {}
        for size in sizes(k):
            bs, _ = le.layout("vandrs", (k, m, 8), size)
            v[size] = (bs, size - (k - 1) * bs)
        assert v[k * 8704 - 15] == (8704, 8704 - 15) and (8704 - 15) % 16 == 1
        assert v[k * 2048 - 16] == (2048, 2032)
        assert v[(k - 1) * 128 * k + 5] == (128 * k, 5)
        if k == 10:
            assert v[1 << 20] == (104960, 103936) and v[(1 << 20) + 1] == (104960, 103937)
            assert [6, 7, 8, 9] in erasures(10, 4) and [0, 1, 2, 9] in erasures(10, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,size", all_shapes(), ids=lambda x: str(x))
def test_gf8_edge_tiles(gpu, le, oracle, k, m, size):
    errs = run_shape(gpu, le, oracle, k, m, size)
    assert not errs, "\n".join(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("wg", ["64", "256"])
def test_gf8_edge_tiles_forced_width(gpu, wg):
    """Every shape with LEOEC_GF8_WG forced, measurement library, own process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LEOEC_LIBRARY="measure", LEOEC_GF8_WG=wg, LIBC_FATAL_STDERR_="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=root, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"gf8 edge tiles wg {wg}: {len(all_shapes())} shapes ok" in r.stdout, r.stdout[-2000:]


def _child():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from leo_erasure_amd import _lib
    from oracle import oracle as O
    assert _lib.is_measure_build(), "the child runs the measurement library"
    assert le.gf_init() == "ok"
    errs = []
    for k, m, size in all_shapes():
        errs += run_shape(torch, le, O, k, m, size)
    for e in errs:
        print("ERROR", e)
    if not errs:
        print(f"gf8 edge tiles wg {os.environ.get('LEOEC_GF8_WG')}: {len(all_shapes())} shapes ok")
    return 1 if errs else 0


if __name__ == "__main__":
    sys.exit(_child())
