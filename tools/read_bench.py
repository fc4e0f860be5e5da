"""leoec_read_dev against what a caller does without it: leoec_decode_dev of
the batch (every erased data block rebuilt in full, in place), then a device
copy of the range.

The method is tools/update_bench.py's: one process on the product library, HIP
events around a window of calls per leg (at least `iters` calls and at least
100 ms), every leg warmed up, the legs alternated round by round in rotating
order.  Batches of 2,048 objects of 1 MiB; per range and erased set two legs:

    read_R_E   leoec_read_dev of the range with the erased set
    ref_R_E    leoec_decode_dev of the batch with the erased set, then
               out[:, lead:lead + L] = objs[:, offset:offset + L] (one strided
               device copy)

Ranges: 4 KiB and 64 KiB inside data block 1 at an odd offset (bs + 5,003), one
block (offset bs), 256 KiB from bs + 5,003 (several blocks), the object.
Erased sets: `one`, data block 1 (inside every range), and `m`, the m data
blocks from 1 up.  Neither side's time depends on the bytes: no kernel branches
on data, and decode never reads the blocks it rebuilds, so the same batch serves
every iteration.

Per leg the median, minimum and maximum milliseconds per call over the rounds,
`spread` = (max - min) / median, and for the read legs `gbps`, the bytes of the
traffic model over the median: (k + 1) L for the bytes of the range in a lost
block, 2 L for those in an intact one.  `read_over_ref_*`: the ratio of the
medians.  `crossover_bytes_*`: the range length at which the two medians meet,
interpolated linearly in L between the last length read wins at and the first
it loses at (null when one side wins everywhere).

The gate: a 4 KiB range inside a lost block must take at most 0.5 of decode +
copy in every config and under both erased sets (the traffic model gives about
0.03; update against copy + encode measured 0.03-0.11 at 4 KiB).  A cell above
it is named on stderr and the exit status is 1.

Before and after the timed rounds every cell is read once from a freshly
encoded batch whose erased blocks were overwritten, and out must hold the
object's bytes.  One JSON line per config.

    python tools/read_bench.py [--rounds 5] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GATE_4K = 0.5  # read / (decode + copy) at most, for a 4 KiB range inside a lost block
CONFIGS = [("vandrs", 10, 4, 8, 1 << 20, 2048), ("vandrs", 10, 4, 16, 1 << 20, 2048),
           ("cauchyrs", 10, 4, 8, 1 << 20, 2048), ("liberation", 4, 2, 7, 1 << 20, 2048)]


def ranges(bs, size):
    """[(name, offset, length)] ascending in length."""
    odd = bs + 5003
    out = [("4k", odd, 4096), ("64k", odd, 65536), ("block", bs, bs), ("256k", odd, 256 << 10),
           ("object", 0, size)]
    assert all(off + length <= size for _, off, length in out)
    return sorted(out, key=lambda p: p[2])


def model_bytes(k, bs, off, length, erased):
    """The traffic model's bytes per object."""
    total, p, end = 0, off, off + length
    while p < end:
        j = p // bs
        q = min(end, (j + 1) * bs)
        total += ((k + 1) if j in erased else 2) * (q - p)
        p = q
    return total


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    objs = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    objs.random_(0, 256)
    parity = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    le.device.encode(cls, p, objs, size, parity)
    out = torch.empty((n, stride + 16), dtype=torch.uint8, device="cuda")
    rlist = ranges(bs, size)
    sets = {"one": [1], "m": list(range(1, 1 + m))}
    legs = [f"{side}_{name}_{e}" for name, _, _ in rlist for e in sets for side in ("read", "ref")]
    where = {name: (off, length) for name, off, length in rlist}

    def call(leg):
        side, name, e = leg.split("_")
        off, length = where[name]
        lead = off % 16
        if side == "read":
            le.device.read(cls, p, objs, size, parity, sets[e], off, length, out=out)
        else:
            le.device.decode(cls, p, objs, size, parity, sets[e])
            out[:, lead:lead + length].copy_(objs[:, off:off + length])

    def check(when):
        objs.random_(0, 256)
        le.device.encode(cls, p, objs, size, parity)
        good = objs.clone()
        for e, ids in sets.items():
            for j in ids:
                objs[:, j * bs:min((j + 1) * bs, size)] = 0xA5
            for name, (off, length) in where.items():
                out.fill_(0x5A)
                call(f"read_{name}_{e}")
                lead = off % 16
                assert torch.equal(out[:, lead:lead + length], good[:, off:off + length]), (cfg, name, e, when)
                assert bool((out[:, :lead] == 0x5A).all()) and bool((out[:, lead + length:] == 0x5A).all()), \
                    (cfg, name, e, when, "outside the range")
        objs.copy_(good)

    check("warm-up")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = {}
    for leg in legs:  # warm-up, and the calls of a timed window: at least `iters`, at least 100 ms
        for _ in range(3):
            call(leg)
        torch.cuda.synchronize()
        start.record()
        for _ in range(5):
            call(leg)
        stop.record()
        torch.cuda.synchronize()
        reps[leg] = max(iters, min(5000, int(100.0 / max(start.elapsed_time(stop) / 5, 1e-3)) + 1))
    ms = {leg: [] for leg in legs}
    for r in range(rounds):
        for i in range(len(legs)):
            leg = legs[(i + r) % len(legs)]
            call(leg)
            torch.cuda.synchronize()
            start.record()
            for _ in range(reps[leg]):
                call(leg)
            stop.record()
            torch.cuda.synchronize()
            ms[leg].append(start.elapsed_time(stop) / reps[leg])
    check("after the timed rounds")
    res = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "legs": {}}
    for leg in legs:
        side, name, e = leg.split("_")
        off, length = where[name]
        med = statistics.median(ms[leg])
        cell = {"bytes": length, "calls": reps[leg], "ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                "ms_max": round(max(ms[leg]), 4), "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4)}
        if side == "read":
            model = n * model_bytes(k, bs, off, length, sets[e])
            cell.update(model_mb=round(model / 1e6, 1), gbps=round(model / med / 1e6, 1))
        res["legs"][leg] = cell
    res["max_spread"] = max(c["spread"] for c in res["legs"].values())
    for e in sets:
        cross, prev = None, None
        for name, _, length in rlist:
            rd, ref = res["legs"][f"read_{name}_{e}"]["ms"], res["legs"][f"ref_{name}_{e}"]["ms"]
            d = rd - ref
            res[f"read_over_ref_{name}_{e}"] = round(rd / ref, 4)
            if cross is None and prev is not None and prev[1] < 0 <= d:
                cross = int(prev[0] + (length - prev[0]) * (-prev[1]) / (d - prev[1]))
            prev = (length, d)
        res[f"crossover_bytes_{e}"] = cross
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    ap.add_argument("--objects-scale", type=float, default=1.0,
                    help="scale every config's object count (rehearsals at a small size)")
    args = ap.parse_args()
    import torch
    import leo_erasure_amd as le
    assert torch.cuda.is_available(), "read_bench needs a GPU"
    torch.cuda.set_device(0)
    assert le.gf_init() == "ok"
    missed = []
    for cfg in CONFIGS:
        cfg = cfg[:5] + (max(128, int(cfg[5] * args.objects_scale)) // 128 * 128,)
        res = run_config(torch, le, cfg, args.rounds, args.iters)
        missed += [(res["config"], e, res[f"read_over_ref_4k_{e}"]) for e in ("one", "m")
                   if res[f"read_over_ref_4k_{e}"] > GATE_4K]
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
    for config, e, ratio in missed:
        print(f"gate missed: {config}, 4 KiB, erased {e}: {ratio} of decode + copy (at most {GATE_4K})",
              file=sys.stderr)
    sys.exit(1 if missed else 0)


if __name__ == "__main__":
    main()
