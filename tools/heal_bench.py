"""leoec_heal_dev against leoec_decode_dev, against its own generic form and
against the traffic it has to move.

One process on the measurement build (libleoec_measure.so), HIP events, every
leg warmed up, the legs alternated round by round in rotating order.
vandrs(10,4,8), 2,048 objects of 1 MiB (or --objects / --size):

    uniform    every object has lost data blocks {0,1,2,3}
        decode       leoec_decode_dev with that erasure (one launch argument)
        heal         leoec_heal_dev, fused form (gf8_heal: per-object lookup)
    scattered  object o has lost block o mod 14 alone
        heal         fused form
        generic      LEOEC_HEAL_FORM=1: masks copied back, one launch per run
                     of equal masks (here: one per object)
    sparse     object o has lost block (o / 64) mod 14 when o mod 64 == 0
        heal         fused form: what the early exit of the clean objects costs

Lost blocks are never read, so no leg needs them re-poisoned between timed
calls; after the timed rounds every (pattern, form) heals a freshly poisoned
batch of the timed size and both arenas must equal the originals byte for
byte.  One JSON line: per leg the median, minimum and maximum milliseconds
per call over the rounds, `spread` = (max - min) / median, the bytes the leg
must move (survivors read + lost blocks written; decode: 10 read, 4 written)
and that traffic's time at 8 TB/s.

    python tools/heal_bench.py [--rounds 7] [--iters 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LEOEC_LIBRARY"] = "measure"  # before the package loads its library

HBM_PEAK = 8.0e12  # bytes / s, MI355X HBM3E spec peak
POISON = 0xA5
CLS, K, M, W = "vandrs", 10, 4, 8


def patterns(n):
    return {"uniform": [0xF] * n,
            "scattered": [1 << (o % (K + M)) for o in range(n)],
            "sparse": [1 << ((o // 64) % (K + M)) if o % 64 == 0 else 0 for o in range(n)]}


def traffic(masks, bs):
    """Blocks a pattern reads (k survivors per damaged object) and writes."""
    damaged = sum(1 for x in masks if x)
    return (K * damaged + sum(bin(x).count("1") for x in masks)) * bs


def run(torch, le, size, n, rounds, iters):
    p = (K, M, W)
    bs, _ = le.layout(CLS, p, size)
    stride = (size + 15) // 16 * 16
    objs = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    objs.random_(0, 256)
    par = torch.empty((n, M * bs), dtype=torch.uint8, device="cuda")
    le.device.encode(CLS, p, objs, size, par)
    torch.cuda.synchronize()
    objs0, par0 = objs.clone(), par.clone()
    pats = patterns(n)
    lost = {name: torch.tensor(m, dtype=torch.int64).to(torch.int32).cuda() for name, m in pats.items()}
    unhealed = torch.empty(n, dtype=torch.int32, device="cuda")
    legs = [("uniform", "decode"), ("uniform", "heal"), ("scattered", "heal"),
            ("scattered", "generic"), ("sparse", "heal")]

    def select(form):
        le._lib.measure_set_knob("LEOEC_HEAL_FORM", "1" if form == "generic" else None)

    def call(pat, form):
        if form == "decode":
            le.device.decode(CLS, p, objs, size, par, [0, 1, 2, 3])
        else:
            le.device.heal(CLS, p, objs, size, par, lost[pat], unhealed=unhealed)

    def poison(pat):
        masks = lost[pat]
        for b in range(K + M):
            rows = ((masks >> b) & 1).nonzero().flatten()
            if rows.numel() == 0:
                continue
            if b < K:
                lo, hi = b * bs, min((b + 1) * bs, size)
                objs[rows, lo:hi] = POISON
            else:
                par[rows, (b - K) * bs:(b - K + 1) * bs] = POISON

    def check(pat, form):
        poison(pat)
        select(form)
        unhealed.fill_(-1)
        call(pat, form)
        torch.cuda.synchronize()
        assert torch.equal(objs, objs0), (pat, form, "objs differ after the heal")
        assert torch.equal(par, par0), (pat, form, "parity differs after the heal")
        if form != "decode":
            assert not bool(unhealed.any()), (pat, form, "unhealed words set")

    for pat, form in legs:  # warm-up: code objects, the pattern table, the plan cache; the answer
        check(pat, form)
        for _ in range(2):
            call(pat, form)
        torch.cuda.synchronize()
    ms = {leg: [] for leg in legs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds):
        for i in range(len(legs)):
            leg = legs[(i + r) % len(legs)]
            select(leg[1])
            call(*leg)
            torch.cuda.synchronize()
            start.record()
            for _ in range(iters):
                call(*leg)
            stop.record()
            torch.cuda.synchronize()
            ms[leg].append(start.elapsed_time(stop) / iters)
    for leg in legs:  # and every timed form heals a damaged batch of the timed size exactly
        check(*leg)
    select("heal")
    out = {"config": "%s(%d,%d,%d)" % (CLS, K, M, W), "size": size, "objects": n, "block_size": bs,
           "rounds": rounds, "iters": iters, "legs": {}}
    for leg in legs:
        med = statistics.median(ms[leg])
        nbytes = traffic(pats[leg[0]], bs)
        out["legs"]["%s/%s" % leg] = {
            "ms": round(med, 4), "ms_min": round(min(ms[leg]), 4), "ms_max": round(max(ms[leg]), 4),
            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4), "bytes": nbytes,
            "model_ms": round(nbytes / HBM_PEAK * 1e3, 4),
            "hbm_share": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
    L = out["legs"]
    out["uniform_heal_over_decode"] = round(L["uniform/heal"]["ms"] / L["uniform/decode"]["ms"], 4)
    out["scattered_generic_over_fused"] = round(L["scattered/generic"]["ms"] / L["scattered/heal"]["ms"], 2)
    out["scattered_fused_over_model"] = round(L["scattered/heal"]["ms"] / L["scattered/heal"]["model_ms"], 3)
    # 1 object in 64 damaged: the scattered leg's time / 64 is what its damaged
    # objects cost; the rest is what the 63 clean ones in 64 cost
    out["sparse_ms_minus_scattered_over_64"] = round(L["sparse/heal"]["ms"] - L["scattered/heal"]["ms"] / 64, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--objects", type=int, default=2048)
    ap.add_argument("--size", type=int, default=1 << 20)
    ap.add_argument("--out", default="", help="also append the JSON line to this file")
    args = ap.parse_args()
    import torch
    import leo_erasure_amd as le
    assert torch.cuda.is_available(), "heal_bench needs a GPU"
    assert le._lib.is_measure_build()
    torch.cuda.set_device(0)
    assert le.gf_init() == "ok"
    line = json.dumps(run(torch, le, args.size, args.objects, args.rounds, args.iters))
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
