"""leoec_read_dev over three objects whose rows lie 2^32 + 48 bytes apart, in a
process of its own (started by
test_device_read.py::test_wide_strides_in_own_process): objs and parity are
regions at fixed offsets of every row of the first half of one 17 GB device
allocation, as in wide_helpers, and the out rows lie in the second half (the
call refuses an out whose extent overlaps that of objs or parity), so
`o * stride` crosses 2^32 and 2^33 for all three buffers with no large data.
Every region is compared with PAD bytes of the allocation's fill on each side,
in every row: a kernel that kept a row offset or a stride in 32 bits would read
row 0's bytes for every object, or write them o * 48 bytes past row 0's region.
The erased blocks (data blocks 1 and 3: intact, lost, intact, lost; coding block 0
where m > 2) hold POISON.

Prints "ok: <n> families" as its last line; any mismatch is an assertion."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import gpu_helpers as H  # noqa: E402
import read_helpers as R  # noqa: E402

STRIDE = 2**32 + 48
NOBJ = 3
PAD = 4096
HALF = 2 * STRIDE + (8 << 20)  # bytes of one extent: three rows
GAP = 64 << 10
FILL = H.GUARD_FILL
FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 20, 4, 8, 8704), ("vandrs", 6, 3, 32, 8704),
            ("cauchyrs", 10, 4, 8, 4352 * 8), ("liberation", 10, 2, 11, 2176 * 11)]


def _up(x, a):
    return (x + a - 1) // a * a


def run(gpu, le, oracle, buf, fam):
    cls, k, m, w, B = fam
    size = k * B - 17
    bs, _ = le.layout(cls, (k, m, w), size)
    off, length = bs - 5, 3 * bs + 12
    erased = [1, 3] + ([k] if m > 2 else [])
    lead = off % 16
    widths = {"objs": size, "parity": m * bs, "out": _up(lead + length, 16)}
    at, cursor = {}, PAD
    for name in ("objs", "parity"):
        at[name] = cursor
        cursor = _up(cursor + widths[name] + PAD + GAP, 16)
    at["out"] = HALF + PAD
    assert max(cursor, widths["out"] + 2 * PAD) < (8 << 20) and buf.numel() >= 2 * HALF
    rng = np.random.Generator(np.random.PCG64(size))
    objs = rng.integers(0, 256, (NOBJ, size), dtype=np.uint8)
    parity = np.stack([np.frombuffer(b"".join(oracle.encode(cls, k, m, w, objs[o].tobytes())[k:]), dtype=np.uint8)
                       for o in range(NOBJ)])
    before = {"objs": objs.copy(), "parity": parity.copy(),
              "out": np.full((NOBJ, widths["out"]), R.OUT_FILL, dtype=np.uint8)}
    for e in erased:
        if e < k:
            before["objs"][:, e * bs:min((e + 1) * bs, size)] = H.POISON
        else:
            before["parity"][:, (e - k) * bs:(e - k + 1) * bs] = H.POISON
    after = {name: rows.copy() for name, rows in before.items()}
    after["out"][:, lead:lead + length] = objs[:, off:off + length]

    def window(name, o):
        lo = o * STRIDE + at[name] - PAD
        return buf[lo:lo + widths[name] + 2 * PAD]

    def image(rows, name, o):
        img = np.full(widths[name] + 2 * PAD, FILL, dtype=np.uint8)
        img[PAD:PAD + widths[name]] = rows[name][o]
        return gpu.from_numpy(img).cuda()

    for name in widths:
        for o in range(NOBJ):
            window(name, o).copy_(image(before, name, o))
    views = {name: gpu.as_strided(buf[at[name]:], (NOBJ, widths[name]), (STRIDE, 1)) for name in widths}
    le.device.read(cls, (k, m, w), views["objs"], size, views["parity"], erased, off, length, out=views["out"])
    gpu.cuda.synchronize()
    for name in widths:
        for o in range(NOBJ):
            got, want = window(name, o), image(after, name, o)
            if not gpu.equal(got, want):
                ne = (got != want).nonzero()
                first = int(ne[0, 0])
                raise AssertionError(f"{fam} [{off}, +{length}): {name} row {o}: {ne.shape[0]} bytes differ, "
                                     f"first at region byte {first - PAD}")
    print(f"{R.family_id(fam)}: ok", flush=True)


def main():
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    oracle.lib()
    assert torch.cuda.is_available() and le.gf_init() == "ok"
    buf = torch.empty(2 * HALF, dtype=torch.uint8, device="cuda")
    for fam in FAMILIES:
        run(torch, le, oracle, buf, fam)
    print(f"ok: {len(FAMILIES)} families")


if __name__ == "__main__":
    main()
