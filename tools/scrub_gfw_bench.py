"""leoec_scrub_gfw_dev on batches of the GF(2^w) word classes against what a
caller had before it: leoec_locate_gfw_dev alone on a clean batch,
leoec_locate_gfw_dev + leoec_heal_dev (which synchronises for these classes)
on a damaged one.

The method is tools/scrub_ws_bench.py's: one process on the measurement build
(libleoec_measure.so), HIP events around `iters` calls per leg, every leg
warmed up, the legs alternated round by round in rotating order.  Batches:

    clean    no object damaged                      scrub_gfw against locate_gfw
    sparse   one object in 64 with one damaged      scrub_gfw against locate_gfw + heal
             data byte
    dense    every object with data block 3         scrub_gfw against locate_gfw + heal
             replaced

Both sides repair in place, so a damaged batch is clean after one call: every
timed iteration of the sparse and dense legs first puts the damage back, the
same for both sides, and the legs `damage_sparse` and `damage_dense` time that
step alone.  `net` is a leg's median less its damage step's.  Both sides get
the same workspace (scrub_gfw the whole of it, locate_gfw its encode region).
Configs: vandrs (10,4,16), (10,4,32) and (20,4,8), 2,048 objects of 1 MiB each
(ragged: the last data block is clipped).

After the timed rounds every leg must answer a freshly damaged batch exactly:
the words, the totals (scrub_gfw) or unhealed (sequence), and every byte back
to the clean batch.  One JSON line per config: per leg the median, minimum and
maximum milliseconds per call over the rounds; `spread` is (max - min) /
median of a leg's rounds; `scrub_over_ref_<batch>` from the net medians.

    python tools/scrub_gfw_bench.py [--rounds 7] [--iters 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LEOEC_LIBRARY"] = "measure"  # before the package loads its library

CONFIGS = [("vandrs", 10, 4, 16, 1 << 20, 2048), ("vandrs", 10, 4, 32, 1 << 20, 2048),
           ("vandrs", 20, 4, 8, 1 << 20, 2048)]
BATCHES = ["clean", "sparse", "dense"]
LEGS = [side + "_" + b for b in BATCHES for side in ("scrub", "ref")] + ["damage_sparse", "damage_dense"]
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
    need = le.device.scrub_gfw_workspace(cls, p, size, n)
    enc = le.device.locate_gfw_workspace(cls, p, size, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ws_enc = ws[need - enc:]
    assert ws_enc.data_ptr() % 16 == 0

    def damage(batch):
        if batch == "sparse":
            work[::64, sparse_pos] = sparse_bytes
        elif batch == "dense":
            work[:, lo:hi] = junk

    def call(leg):
        side, batch = leg.split("_")
        damage(batch)
        if side == "scrub":
            le.device.scrub_gfw(cls, p, work, size, par, report=words, totals=totals, workspace=ws)
        elif side == "ref":
            le.device.locate_gfw(cls, p, work, size, par, lost=words, workspace=ws_enc)
            if batch != "clean":
                le.device.heal(cls, p, work, size, par, words, unhealed=unhealed)

    def check(leg, when):
        side, batch = leg.split("_")
        if side == "damage":
            return
        words.fill_(-1)
        totals.fill_(-1)
        unhealed.fill_(0 if batch == "clean" else -1)
        call(leg)
        torch.cuda.synchronize()
        assert torch.equal(words.cpu(), want[batch]), (cfg, leg, when, "words")
        assert torch.equal(work, clean), (cfg, leg, when, "bytes")
        if side == "scrub":
            assert totals.tolist() == [int((want[batch] != 0).sum()), 0], (cfg, leg, when, totals.tolist())
        else:
            assert not unhealed.any(), (cfg, leg, when, "unhealed")

    for leg in LEGS:  # warm-up: code objects, the block table; and the answer
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
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "workspace": need, "legs": {}}
    for leg in LEGS:
        med = statistics.median(ms[leg])
        out["legs"][leg] = {"ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4)}
    for batch in BATCHES:
        base = out["legs"]["damage_" + batch]["ms"] if batch != "clean" else 0.0
        net = {side: out["legs"][side + "_" + batch]["ms"] - base for side in ("scrub", "ref")}
        for side in net:
            out["legs"][side + "_" + batch]["net"] = round(net[side], 4)
        out["scrub_over_ref_" + batch] = round(net["scrub"] / net["ref"], 4)
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
    assert torch.cuda.is_available(), "scrub_gfw_bench needs a GPU"
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
