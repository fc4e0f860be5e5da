"""leoec_update_dev against what a caller does without it: a device copy of
the patch into objs, then leoec_encode_dev of the whole object.

The method is tools/heal_ws_bench.py's: one process on the product library,
HIP events around a window of calls per leg (at least `iters` calls and at
least 100 ms), every leg warmed up, the legs alternated round by round in
rotating order.  Batches of 2,048 objects of 1 MiB; per patch length L two legs:

    upd_L   leoec_update_dev of [offset, offset + L) of every object
    ref_L   objs[:, offset:offset + L] = patch (one strided device copy), then
            leoec_encode_dev of the batch

Lengths: 4 KiB and 64 KiB inside data block 1 at an odd offset (bs + 5,003),
one block (offset bs), the whole object, and 128 / 256 / 512 KiB from
bs + 5,003 (several blocks) to bracket the crossover.  Neither side's time
depends on the bytes: no kernel branches on data, so the same patch is applied
in every iteration.

Per leg the median, minimum and maximum milliseconds per call over the rounds,
`spread` = (max - min) / median, and `gbps`, the bytes of the traffic model
over the median: update (3 + 2m) L per object (old, new and the stored new
bytes, m coding columns read and written), the reference 2 L + size + m bs
(the copy, the object read, the coding blocks written).  `crossover_bytes`:
the patch length at which the two medians meet, interpolated linearly in L
between the last length update wins at and the first it loses at (null when
one side wins everywhere).

After the timed rounds the batch is re-encoded, every length is applied once
and the stripes must verify clean with the patch in place.  One JSON line per
config.

    python tools/update_bench.py [--rounds 5] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = [("vandrs", 10, 4, 8, 1 << 20, 2048), ("vandrs", 10, 4, 16, 1 << 20, 2048),
           ("cauchyrs", 10, 4, 8, 1 << 20, 2048), ("liberation", 4, 2, 7, 1 << 20, 2048)]


def patches(bs, size):
    """[(name, offset, length)] ascending in length."""
    odd = bs + 5003
    out = [("4k", odd, 4096), ("64k", odd, 65536), ("block", bs, bs), ("128k", odd, 128 << 10),
           ("256k", odd, 256 << 10), ("512k", odd, 512 << 10), ("object", 0, size)]
    assert all(off + length <= size for _, off, length in out)
    return sorted(out, key=lambda p: p[2])


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    objs = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    objs.random_(0, 256)
    parity = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    patch = torch.empty((n, stride + 16), dtype=torch.uint8, device="cuda")
    patch.random_(0, 256)
    plist = patches(bs, size)
    legs = [side + "_" + name for name, _, _ in plist for side in ("upd", "ref")]
    where = {name: (off, length) for name, off, length in plist}

    def call(leg):
        side, name = leg.split("_")
        off, length = where[name]
        lead = off % 16
        if side == "upd":
            le.device.update(cls, p, objs, size, parity, patch, off, length)
        else:
            objs[:, off:off + length].copy_(patch[:, lead:lead + length])
            le.device.encode(cls, p, objs, size, parity)

    def check(when):
        for name, (off, length) in where.items():
            objs.random_(0, 256)
            le.device.encode(cls, p, objs, size, parity)
            call("upd_" + name)
            flags = le.device.verify(cls, p, objs, size, parity)
            assert not flags.any(), (cfg, name, when, "verify")
            assert torch.equal(objs[:, off:off + length], patch[:, off % 16:off % 16 + length]), (cfg, name, when)

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
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "legs": {}}
    for leg in legs:
        side, name = leg.split("_")
        length = where[name][1]
        model = n * ((3 + 2 * m) * length if side == "upd" else 2 * length + size + m * bs)
        med = statistics.median(ms[leg])
        out["legs"][leg] = {"bytes": length, "calls": reps[leg], "ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4),
                            "model_mb": round(model / 1e6, 1), "gbps": round(model / med / 1e6, 1)}
    cross, prev = None, None
    for name, _, length in plist:
        d = out["legs"]["upd_" + name]["ms"] - out["legs"]["ref_" + name]["ms"]
        out["upd_over_ref_" + name] = round(out["legs"]["upd_" + name]["ms"] / out["legs"]["ref_" + name]["ms"], 4)
        if cross is None and prev is not None and prev[1] < 0 <= d:
            cross = int(prev[0] + (length - prev[0]) * (-prev[1]) / (d - prev[1]))
        prev = (length, d)
    out["crossover_bytes"] = cross
    return out


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
    assert torch.cuda.is_available(), "update_bench needs a GPU"
    torch.cuda.set_device(0)
    assert le.gf_init() == "ok"
    for cfg in CONFIGS:
        cfg = cfg[:5] + (max(128, int(cfg[5] * args.objects_scale)) // 128 * 128,)
        line = json.dumps(run_config(torch, le, cfg, args.rounds, args.iters))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
