"""leoec_locate_gfw_dev (the GF(2^w) word classes) against two-pass
leoec_verify_dev, and its dirty branch.

One process on the measurement build (libleoec_measure.so), HIP events, every
leg warmed up, the legs alternated round by round in rotating order (the
conditions of tools/locate_ws_bench.py), one workspace of the query's size
shared by every leg:

    verify             leoec_verify_dev (encode + verify_compare) on clean stripes
    locate_gfw         leoec_locate_gfw_dev on the same clean stripes: the same
                       encode, gfw_locate reading what verify_compare reads,
                       plus a memset and a nobj-word launch
    locate_gfw_sparse  one object in 64 with one damaged data byte
    locate_gfw_dirty   every object with one whole data block replaced: every
                       wave of every object takes the dirty branch

After the timed rounds every leg must answer a damaged batch of the timed
size exactly.  One JSON line per config: per leg the median, minimum and
maximum milliseconds per call over the rounds; `spread` is (max - min) /
median of a leg's rounds, the yardstick for a difference between legs.

    python tools/locate_gfw_bench.py [--rounds 7] [--iters 100] [--out FILE]
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
LEGS = ["verify", "locate_gfw", "locate_gfw_sparse", "locate_gfw_dirty"]
DIRTY_BLOCK = 3  # the data block locate_gfw_dirty replaces


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    clean = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    clean.random_(0, 256)
    par = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    le.device.encode(cls, p, clean, size, par)
    need = le.device.locate_gfw_workspace(cls, p, size, n)
    assert need == n * m * bs == le.device.verify_workspace(cls, p, size, n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sparse, dirty = clean.clone(), clean.clone()
    sparse_pos = (size - 1) // 2
    sparse[::64, sparse_pos] ^= 0x10
    lo, hi = DIRTY_BLOCK * bs, min((DIRTY_BLOCK + 1) * bs, size)
    dirty[:, lo:hi] ^= torch.randint(1, 256, (n, hi - lo), dtype=torch.uint8, device="cuda")
    objs = {"verify": clean, "locate_gfw": clean, "locate_gfw_sparse": sparse,
            "locate_gfw_dirty": dirty}
    words = torch.empty(n, dtype=torch.int32, device="cuda")
    zeros = torch.zeros(n, dtype=torch.int32)
    want = {"verify": zeros, "locate_gfw": zeros, "locate_gfw_sparse": zeros.clone(),
            "locate_gfw_dirty": torch.full((n,), 1 << DIRTY_BLOCK, dtype=torch.int32)}
    want["locate_gfw_sparse"][::64] = 1 << (sparse_pos // bs)

    def call(leg):
        if leg == "verify":
            le.device.verify(cls, p, objs[leg], size, par, flags=words, workspace=ws)
        else:
            le.device.locate_gfw(cls, p, objs[leg], size, par, lost=words, workspace=ws)

    def answer(leg):
        call(leg)
        torch.cuda.synchronize()
        return words.cpu()

    for leg in LEGS:  # warm-up: code objects, the code's table; and the answer
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
        assert torch.equal(answer("locate_gfw"), lost), (cfg, "locate_gfw",
                                                         words.cpu()[[0, n - 1]].tolist())
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "workspace": need, "rounds": rounds, "iters": iters, "legs": {}}
    for leg in LEGS:
        med = statistics.median(ms[leg])
        out["legs"][leg] = {"ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4)}
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
    assert torch.cuda.is_available(), "locate_gfw_bench needs a GPU"
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
