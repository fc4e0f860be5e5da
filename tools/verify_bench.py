"""leoec_verify_dev against leoec_encode_dev and against its own two-pass form.

One process on the measurement build (libleoec_measure.so), HIP events, every
leg warmed up, the legs alternated round by round in rotating order:

    encode     leoec_encode_dev of the same batch (reads k, writes m blocks)
    verify     the shipped form: gf8_check where it serves (reads k + m
               blocks), else two-pass
    two_pass   LEOEC_VERIFY_FORM=1: encode into a workspace, then compare
               (reads k + m, writes m, reads m more: k + 3m blocks)
    verify_w5  LEOEC_VERIFY_FORM=2: gf8_check<10,4> under a 5-wave register
               budget (fused configurations only)

Every verify runs on clean stripes (the encode's own output) and must report
none damaged.  One JSON line per config: per leg the median, minimum and
maximum milliseconds per call over the rounds, the algorithmic bytes computed
from the shapes and the median's share of 8 TB/s; `spread` is (max - min) /
median of a leg's rounds, the yardstick for a difference between legs.

    python tools/verify_bench.py [--rounds 7] [--iters 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["LEOEC_LIBRARY"] = "measure"  # before the package loads its library

HBM_PEAK = 8.0e12  # bytes / s, MI355X HBM3E spec peak
CONFIGS = [("vandrs", 10, 4, 8, 1 << 20, 2048), ("vandrs", 10, 4, 8, 64 << 20, 64),
           ("cauchyrs", 10, 4, 8, 1 << 20, 2048)]
FORM = {"verify": None, "two_pass": "1", "verify_w5": "2"}


def algorithmic_bytes(leg, k, m, bs, n):
    blocks = {"encode": k + m, "verify": k + m, "verify_w5": k + m, "two_pass": k + 3 * m}[leg]
    return blocks * bs * n


def run_config(torch, le, cfg, rounds, iters):
    cls, k, m, w, size, n = cfg
    p = (k, m, w)
    bs, _ = le.layout(cls, p, size)
    stride = (size + 15) // 16 * 16
    objs = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    objs.random_(0, 256)
    par = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")
    scratch = torch.empty((n, m * bs), dtype=torch.uint8, device="cuda")  # the timed encode's output
    flags = torch.empty(n, dtype=torch.int32, device="cuda")
    fused = le.device.verify_workspace(cls, p, size, n) == 0
    ws = torch.empty(n * m * bs, dtype=torch.uint8, device="cuda")
    legs = ["encode", "verify", "two_pass"] + (["verify_w5"] if fused and (k, m) == (10, 4) else [])
    if not fused:
        legs.remove("two_pass")  # the shipped form is the two-pass form

    def call(leg):
        if leg == "encode":
            le.device.encode(cls, p, objs, size, scratch)
        else:
            le.device.verify(cls, p, objs, size, par, flags=flags, workspace=ws)

    def select(leg):
        if leg != "encode":
            le._lib.measure_set_knob("LEOEC_VERIFY_FORM", FORM[leg])

    le.device.encode(cls, p, objs, size, par)
    for leg in legs:  # warm-up: code objects, the plan cache; and the answer
        select(leg)
        for _ in range(3):
            call(leg)
        torch.cuda.synchronize()
        if leg != "encode":
            assert not bool(flags.any()), (cfg, leg, "clean stripes reported damaged")
    ms = {leg: [] for leg in legs}
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds):
        for i in range(len(legs)):
            leg = legs[(i + r) % len(legs)]
            select(leg)
            call(leg)
            torch.cuda.synchronize()
            start.record()
            for _ in range(iters):
                call(leg)
            stop.record()
            torch.cuda.synchronize()
            ms[leg].append(start.elapsed_time(stop) / iters)
    assert not bool(flags.any()), (cfg, "clean stripes reported damaged")
    if n >= 2:  # and every timed form sees damage at the timed size
        objs[0, size - 1] ^= 1
        par[n - 1, m * bs - 1] ^= 1
        want = torch.zeros(n, dtype=torch.int32)
        want[0], want[n - 1] = (1 << m) - 1, 1 << (m - 1)
        for leg in legs[1:]:
            select(leg)
            call(leg)
            torch.cuda.synchronize()
            assert torch.equal(flags.cpu(), want), (cfg, leg, flags.cpu()[[0, n - 1]].tolist())
    le._lib.measure_set_knob("LEOEC_VERIFY_FORM", None)
    out = {"config": "%s(%d,%d,%d)" % (cls, k, m, w), "size": size, "objects": n, "block_size": bs,
           "shipped_form": "fused" if fused else "two_pass", "rounds": rounds, "iters": iters,
           "legs": {}}
    for leg in legs:
        med = statistics.median(ms[leg])
        nbytes = algorithmic_bytes("two_pass" if leg == "verify" and not fused else leg, k, m, bs, n)
        out["legs"][leg] = {"ms": round(med, 4), "ms_min": round(min(ms[leg]), 4),
                            "ms_max": round(max(ms[leg]), 4),
                            "spread": round((max(ms[leg]) - min(ms[leg])) / med, 4),
                            "bytes": nbytes,
                            "hbm_share": round(nbytes / (med * 1e-3) / HBM_PEAK, 4)}
    enc = out["legs"]["encode"]["ms"]
    out["verify_over_encode"] = round(out["legs"]["verify"]["ms"] / enc, 4)
    if "two_pass" in out["legs"]:
        out["two_pass_over_fused"] = round(out["legs"]["two_pass"]["ms"] / out["legs"]["verify"]["ms"], 4)
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
    assert torch.cuda.is_available(), "verify_bench needs a GPU"
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
