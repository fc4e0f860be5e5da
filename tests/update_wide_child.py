"""leoec_update_dev over three objects whose rows lie 2^32 + 48 bytes apart,
in a process of its own (started by
test_device_update.py::test_wide_strides_in_own_process): objs and parity are
regions at fixed offsets of every row of the first half of one 17 GB device
allocation, as in wide_helpers, and the patch rows lie in the second half (the
call refuses a patch whose extent overlaps that of objs or parity), so
`o * stride` crosses 2^32 and 2^33 for all three buffers with no large data.
Every region is compared with PAD bytes of the allocation's fill on each side,
in every row: a kernel that kept a row offset or a stride in 32 bits would
patch bytes o * 48 past the region of row 0 and leave rows 1 and 2 as they
were.

Prints "ok: <n> families" as its last line; any mismatch is an assertion."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import gpu_helpers as H  # noqa: E402
import update_helpers as U  # noqa: E402

STRIDE = 2**32 + 48
NOBJ = 3
PAD = 4096
HALF = 2 * STRIDE + (8 << 20)  # bytes of one extent: three rows
GAP = 64 << 10
FILL = H.GUARD_FILL
FAMILIES = [("vandrs", 10, 4, 8, 8704), ("vandrs", 6, 3, 32, 8704), ("cauchyrs", 10, 4, 8, 4352 * 8),
            ("liberation", 4, 2, 7, 2176 * 7)]


def _up(x, a):
    return (x + a - 1) // a * a


def run(gpu, le, oracle, buf, fam):
    cls, k, m, w, B = fam
    size = k * B - 17
    bs, _ = le.layout(cls, (k, m, w), size)
    off, length = bs - 5, 2 * bs + 12
    lead = off % 16
    widths = {"objs": size, "parity": m * bs, "patch": lead + length}
    at, cursor = {}, PAD
    for name in ("objs", "parity"):
        at[name] = cursor
        cursor = _up(cursor + widths[name] + PAD + GAP, 16)
    at["patch"] = HALF + PAD
    assert max(cursor, widths["patch"] + 2 * PAD) < (8 << 20) and buf.numel() >= 2 * HALF
    rng = np.random.Generator(np.random.PCG64(size))
    before = {name: rng.integers(0, 256, (NOBJ, widths[name]), dtype=np.uint8) for name in widths}
    pat = U.pattern(length)
    before["patch"][:, :lead] = U.PATCH_FILL
    before["patch"][:, lead:] = before["objs"][:, off:off + length] ^ pat
    d = np.zeros(size, dtype=np.uint8)
    d[off:off + length] = pat
    enc = np.frombuffer(b"".join(oracle.encode(cls, k, m, w, d.tobytes())[k:]), dtype=np.uint8)
    after = {name: rows.copy() for name, rows in before.items()}
    after["objs"][:, off:off + length] ^= pat
    after["parity"] ^= enc[None, :]

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
    le.device.update(cls, (k, m, w), views["objs"], size, views["parity"], views["patch"], off, length)
    gpu.cuda.synchronize()
    for name in widths:
        for o in range(NOBJ):
            got, want = window(name, o), image(after, name, o)
            if not gpu.equal(got, want):
                ne = (got != want).nonzero()
                first = int(ne[0, 0])
                raise AssertionError(f"{fam} [{off}, +{length}): {name} row {o}: {ne.shape[0]} bytes differ, "
                                     f"first at region byte {first - PAD}")
    print(f"{U.family_id(fam)}: ok", flush=True)


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
