"""leoec_locate_dev against leoec_verify_dev, and its dirty branch.

One process on the measurement build (libleoec_measure.so), HIP events, every
leg warmed up, the legs alternated round by round in rotating order (the
conditions of tools/verify_bench.py):

    verify         leoec_verify_dev (gf8_check) on clean stripes
    locate         leoec_locate_dev on the same clean stripes: the same loads
                   and arithmetic plus a memset and a nobj-word launch
    locate_sparse  one object in 64 with one damaged data byte
    locate_dirty   every object with one whole data block replaced: every
                   wave of every object takes the dirty branch

After the timed rounds every leg must answer a damaged batch of the timed
size exactly.  One JSON line per config: per leg the median, minimum and
maximum milliseconds per call over the rounds, the algorithmic bytes (k + m
blocks read) and the median's share of 8 TB/s; `spread` is (max - min) /
median of a leg's rounds, the yardstick for a difference between legs.

    python tools/locate_bench.py [--rounds 7] [--iters 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LEOEC_LIBRARY"] = "measure"  # before the package loads its library

HBM_PEAK = 8.0e12  # bytes / s, MI355X HBM3E spec peak
CONFIGS = [("vandrs", 10, 4, 8, 1 << 20, 2048), ("vandrs", 10, 4, 8, 64 << 20, 64)]
LEGS = ["verify", "locate", "locate_sparse", "locate_dirty"]
DIRTY_BLOCK = 3  # the data block locate_dirty replaces


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    clean = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    clean.random_(0, 256)
    par = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    le.device.encode(cls, p, clean, size, par)
    sparse, dirty = clean.clone(), clean.clone()
    sparse_pos = (size - 1) // 2
    sparse[::64, sparse_pos] ^= 0x10
    lo, hi = DIRTY_BLOCK * bs, min((DIRTY_BLOCK + 1) * bs, size)
    dirty[:, lo:hi] ^= torch.randint(1, 256, (n, hi - lo), dtype=torch.uint8, device="cuda")
    objs = {"verify": clean, "locate": clean, "locate_sparse": sparse, "locate_dirty": dirty}
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    zeros = torch.zeros(n, dtype=torch.int32)
    want = {"verify": zeros, "locate": zeros, "locate_sparse": zeros.clone(),
            "locate_dirty": torch.full((n,), 1 << DIRTY_BLOCK, dtype=torch.int32)}
    want["locate_sparse"][::64] = 1 << (sparse_pos // bs)

    def call(leg):
        if leg == "verify":
            le.device.verify(cls, p, objs[leg], size, par, flags=words)
        else:
            le.device.locate(cls, p, objs[leg], size, par, lost=words)

    def answer(leg):
        call(leg)
        torch.cuda.synchronize()
        return words.cpu()

    for leg in LEGS:  # warm-up: code objects; and the answer
        for _ in range(3):
            call(leg)
        assert torch.equal(answer(leg), want[leg]), (cfg, leg, "warm-up answer")
    ms = {leg: [] for leg in LEGS}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds):
        for i in range(len(LEGS)):
            leg = LEGS[(i + r) % len(LEGS)]
            call(leg)
            torch.cuda.synchronize()
            start.record()
            for _ in range(iters):
                call(leg)
            stop.record()
            torch.cuda.synchronize()
            ms[leg].append(start.elapsed_time(stop) / iters)
    for leg in LEGS:
        assert torch.equal(answer(leg), want[leg]), (cfg, leg, "answer after the timed rounds")
    if n >= 2:  # and the clean legs see damage at the timed size
        clean[0, size - 1] ^= 1
        par[n - 1, m * bs - 1] ^= 1
        flags, lost = zeros.clone(), zeros.clone()
        flags[0], flags[n - 1] = (1 << m) - 1, 1 << (m - 1)
        lost[0], lost[n - 1] = 1 << ((size - 1) // bs), 1 << (k + m - 1)
        assert torch.equal(answer("verify"), flags), (cfg, "verify", words.cpu()[[0, n - 1]].tolist())
        assert torch.equal(answer("locate"), lost), (cfg, "locate", words.cpu()[[0, n - 1]].tolist())
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "legs": {}}
    nbytes = (k + m) * bs * n
    for leg in LEGS:
        med = statistics.median(ms[leg])
        out["legs"][leg] = {"ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4),
                            "bytes": nbytes,
                            "hbm_share": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
    ver = out["legs"]["verify"]["ms"]
    for leg in LEGS[1:]:
        out[leg + "_over_verify"] = round(out["legs"][leg]["ms"] / ver, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    ap.add_argument("--objects-scale", type=float, default=1.0,
                    help="scale every config's object count (rehearsals at a small size)")
    args = ap.parse_args()
    import torch
    import leo_erasure_amd as le
    assert torch.cuda.is_available(), "locate_bench needs a GPU"
    assert le._lib.is_measure_build()
    torch.cuda.set_device(0)
    assert le.gf_init() == "ok"
    for cfg in CONFIGS:
        cfg = cfg[:5] + (max(1, int(cfg[5] * args.objects_scale)),)
        line = json.dumps(run_config(torch, le, cfg, args.rounds, args.iters))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
