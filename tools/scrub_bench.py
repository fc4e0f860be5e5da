"""leoec_scrub_dev against the two-call sequence leoec_locate_dev +
leoec_heal_dev.

One process on the measurement build (libleoec_measure.so), HIP events, every
leg warmed up, the legs alternated round by round in rotating order (the
conditions of tools/locate_bench.py).  Three batches, each through both:

    clean    no object damaged
    sparse   one object in 64 with one damaged data byte
    dense    every object with data block 3 replaced

Both repair in place, so a damaged batch is clean after one call: every timed
iteration of the sparse and dense legs first puts the damage back (one strided
byte copy; one copy of a block per object), the same for both sides, and the
legs `damage_sparse` and `damage_dense` time that step alone.  `net` is a
leg's median less its damage step's.

After the timed rounds every leg must answer a freshly damaged batch exactly:
the words, the totals (scrub) or unhealed (sequence), and every byte back to
the clean batch.  One JSON line per config: per leg the median, minimum and
maximum milliseconds per call over the rounds; `spread` is (max - min) /
median of a leg's rounds, the yardstick for a difference between legs;
`scrub_over_seq` per batch from the net medians.

    python tools/scrub_bench.py [--rounds 7] [--iters 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LEOEC_LIBRARY"] = "measure"  # before the package loads its library

CONFIGS = [("vandrs", 10, 4, 8, 1 << 20, 2048)]
BATCHES = ["clean", "sparse", "dense"]
LEGS = [side + "_" + b for b in BATCHES for side in ("scrub", "seq")] + ["damage_sparse", "damage_dense"]
DENSE_BLOCK = 3  # the data block the dense batch replaces


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    clean = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    clean.random_(0, 256)
    par = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    le.device.encode(cls, p, clean, size, par)
    work = clean.clone()  # the batch every leg runs on
    sparse_pos = (size - 1) // 2
    sparse_bytes = clean[::64, sparse_pos] ^ 0x10
    lo, hi = DENSE_BLOCK * bs, min((DENSE_BLOCK + 1) * bs, size)
    junk = clean[:, lo:hi] ^ torch.randint(1, 256, (n, hi - lo), dtype=torch.uint8, device="cuda")
    zeros = torch.zeros(n, dtype=torch.int32)
    want = {"clean": zeros, "sparse": zeros.clone(),
            "dense": torch.full((n,), 1 << DENSE_BLOCK, dtype=torch.int32)}
    want["sparse"][::64] = 1 << (sparse_pos // bs)
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    unhealed = torch.empty(n, dtype=torch.int32, device="cuda")
    totals = torch.empty(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(le.device.scrub_workspace(cls, p, size, n), dtype=torch.uint8, device="cuda")

    def damage(batch):
        if batch == "sparse":
            work[::64, sparse_pos] = sparse_bytes
        elif batch == "dense":
            work[:, lo:hi] = junk

    def call(leg):
        side, batch = leg.split("_")
        damage(batch)
        if side == "scrub":
            le.device.scrub(cls, p, work, size, par, report=words, totals=totals, workspace=ws)
        elif side == "seq":
            le.device.locate(cls, p, work, size, par, lost=words)
            le.device.heal(cls, p, work, size, par, words, unhealed=unhealed)

    def check(leg, when):
        side, batch = leg.split("_")
        if side == "damage":
            return
        words.fill_(-1)
        totals.fill_(-1)
        unhealed.fill_(-1)
        call(leg)
        torch.cuda.synchronize()
        assert torch.equal(words.cpu(), want[batch]), (cfg, leg, when, "words")
        assert torch.equal(work, clean), (cfg, leg, when, "bytes")
        if side == "scrub":
            assert totals.tolist() == [int((want[batch] != 0).sum()), 0], (cfg, leg, when, totals.tolist())
        else:
            assert not unhealed.any(), (cfg, leg, when, "unhealed")

    for leg in LEGS:  # warm-up: code objects, heal's table; and the answer
        for _ in range(3):
            call(leg)
        check(leg, "warm-up")
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
    work.copy_(clean)
    for leg in LEGS:
        check(leg, "after the timed rounds")
    # and a batch none of the timed ones was: coding block m - 1 of the last
    # object, the last data byte of the first, two blocks of the second
    if n >= 3:
        for side in ("scrub", "seq"):
            par_keep = par.clone()
            work[0, size - 1] ^= 1
            par[n - 1, m * bs - 1] ^= 1
            work[1, 0] ^= 1
            par[1, 0] ^= 1
            call(side + "_clean")
            torch.cuda.synchronize()
            lost = zeros.clone()
            lost[0], lost[n - 1], lost[1] = 1 << ((size - 1) // bs), 1 << (k + m - 1), -(1 << 31)
            assert torch.equal(words.cpu(), lost), (cfg, side, words.cpu()[[0, 1, n - 1]].tolist())
            if side == "scrub":
                assert totals.tolist() == [2, 1], (cfg, totals.tolist())
            work[1, 0] ^= 1
            par[1, 0] ^= 1
            assert torch.equal(work, clean) and torch.equal(par, par_keep), (cfg, side, "bytes")
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "legs": {}}
    for leg in LEGS:
        med = statistics.median(ms[leg])
        out["legs"][leg] = {"ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4)}
    for batch in BATCHES:
        base = out["legs"]["damage_" + batch]["ms"] if batch != "clean" else 0.0
        net = {side: out["legs"][side + "_" + batch]["ms"] - base for side in ("scrub", "seq")}
        for side in net:
            out["legs"][side + "_" + batch]["net"] = round(net[side], 4)
        out["scrub_over_seq_" + batch] = round(net["scrub"] / net["seq"], 4)
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
    assert torch.cuda.is_available(), "scrub_bench needs a GPU"
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
