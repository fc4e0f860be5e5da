"""leoec_heal_ws_dev against leoec_heal_dev on device batches with the caller's
own masks.

The method is tools/scrub_gfw_bench.py's: one process on the measurement build
(libleoec_measure.so), HIP events around `iters` calls per leg, every leg
warmed up, the legs alternated round by round in rotating order.  Batches of
2,048 objects of 1 MiB (ragged: the last data block is clipped):

    clean    no object has lost anything
    sparse   32 objects (every 64th) with two lost blocks each, {1, k} and
             {0, 2} alternating: no two neighbours share a mask
    dense2   every object with the mask {1, k}
    densem   every object with its first m data blocks lost

Both sides rebuild in place and never read a lost block, so the damage is what
the check needs, not what the call does: every timed iteration first poisons
the lost blocks, the same for both sides, and the legs `damage_<batch>` time
that step alone.  `net` is a leg's median less its damage step's.  Configs:
vandrs(10,4,8) (leoec_heal_dev's one-launch family), vandrs(10,4,16),
cauchyrs(10,4,8) and vandrs(20,4,8) (leoec_heal_dev synchronises).

After the timed rounds every leg must answer a freshly poisoned batch exactly:
unhealed, the totals (heal_ws) and every byte back to the clean batch.  One
JSON line per config: per leg the median, minimum and maximum milliseconds per
call over the rounds; `spread` is (max - min) / median of a leg's rounds;
`ws_over_ref_<batch>` from the net medians.

    python tools/heal_ws_bench.py [--rounds 7] [--iters 50] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LEOEC_LIBRARY"] = "measure"  # before the package loads its library

CONFIGS = [("vandrs", 10, 4, 8, 1 << 20, 2048), ("vandrs", 10, 4, 16, 1 << 20, 2048),
           ("cauchyrs", 10, 4, 8, 1 << 20, 2048), ("vandrs", 20, 4, 8, 1 << 20, 2048)]
BATCHES = ["clean", "sparse", "dense2", "densem"]
LEGS = [side + "_" + b for b in BATCHES for side in ("ws", "ref")] + \
    ["damage_" + b for b in BATCHES[1:]]
POISON = 0xA5


def bits(ids):
    return sum(1 << b for b in ids)


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    clean = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    clean.random_(0, 256)
    par_clean = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    le.device.encode(cls, p, clean, size, par_clean)
    work, par = clean.clone(), par_clean.clone()  # the batch every leg runs on
    pairs = [[1, k], [0, 2]]
    # batch -> [(objects, lost ids)]
    groups = {"clean": [],
              "sparse": [(slice(64 * j, None, 128), pairs[j]) for j in (0, 1)],
              "dense2": [(slice(None), pairs[0])],
              "densem": [(slice(None), list(range(m)))]}
    masks = {}
    for batch, gs in groups.items():
        mk = torch.zeros(n, dtype=torch.int32)
        for objs, ids in gs:
            mk[objs] = bits(ids)
        masks[batch] = mk.cuda()
    assert int((masks["sparse"] != 0).sum()) == n // 64
    assert all(int(masks["sparse"][64 * i]) != int(masks["sparse"][64 * i + 64]) for i in range(n // 64 - 1))
    unhealed = torch.empty(n, dtype=torch.int32, device="cuda")
    totals = torch.empty(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(le.device.heal_ws_workspace(cls, p, size, n), dtype=torch.uint8, device="cuda")

    def damage(batch):
        for objs, ids in groups[batch]:
            for b in ids:
                if b < k:
                    work[objs, b * bs:min((b + 1) * bs, size)] = POISON
                else:
                    par[objs, (b - k) * bs:(b - k + 1) * bs] = POISON

    def call(leg):
        side, batch = leg.split("_")
        damage(batch)
        if side == "ws":
            le.device.heal_ws(cls, p, work, size, par, masks[batch], unhealed=unhealed, totals=totals,
                              workspace=ws)
        elif side == "ref":
            le.device.heal(cls, p, work, size, par, masks[batch], unhealed=unhealed)

    def check(leg, when):
        side, batch = leg.split("_")
        if side == "damage":
            return
        unhealed.fill_(-1)
        totals.fill_(-1)
        call(leg)
        torch.cuda.synchronize()
        assert not unhealed.any(), (cfg, leg, when, "unhealed")
        assert torch.equal(work, clean), (cfg, leg, when, "objs")
        assert torch.equal(par, par_clean), (cfg, leg, when, "parity")
        if side == "ws":
            assert totals.tolist() == [int((masks[batch] != 0).sum()), 0], (cfg, leg, when, totals.tolist())

    for leg in LEGS:  # warm-up: code objects, the tables; and the answer
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
    work.copy_(clean)  # (a damage leg ran last)
    par.copy_(par_clean)
    for leg in LEGS:
        check(leg, "after the timed rounds")
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "legs": {}}
    for leg in LEGS:
        med = statistics.median(ms[leg])
        out["legs"][leg] = {"ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4)}
    for batch in BATCHES:
        base = out["legs"]["damage_" + batch]["ms"] if batch != "clean" else 0.0
        net = {side: out["legs"][side + "_" + batch]["ms"] - base for side in ("ws", "ref")}
        for side in net:
            out["legs"][side + "_" + batch]["net"] = round(net[side], 4)
        out["ws_over_ref_" + batch] = round(net["ws"] / net["ref"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    ap.add_argument("--objects-scale", type=float, default=1.0,
                    help="scale every config's object count (rehearsals at a small size)")
    args = ap.parse_args()
    import torch
    import leo_erasure_amd as le
    assert torch.cuda.is_available(), "heal_ws_bench needs a GPU"
    assert le._lib.is_measure_build()
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
