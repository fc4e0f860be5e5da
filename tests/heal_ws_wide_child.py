"""leoec_heal_ws_dev over rows more than 4 GiB apart, in one fresh process: a
plain script, run by test_device_heal_ws.py::
test_heal_ws_wide_strides_in_own_process, as wide_strides_child.py runs
leoec_heal_dev's cases.

Three objects whose rows lie 2^32 + 48 bytes apart in one device allocation of
this process's own (wide_helpers' arena, plans and comparison): object 0
clean, a data and a coding block of object 1, the last m data blocks of object
2 (wide_helpers.heal_masks), for one word family and one packet family, so the
rebuild kernels' obj x stride products are taken in 64 bits.  One JSON line
per case ({"case", "errors", "seconds"}) and a last one with the count; exit
status 3 when the allocation cannot be made.  The first exception ends the
script: nothing more is started on the device after a failed call.

Usage: python tests/heal_ws_wide_child.py"""
import json
import os
import sys
import time

FAMILIES = [("vandrs", 10, 4, 16, 8704), ("cauchyrs", 6, 3, 4, 4352 * 4)]


def plan_heal_ws(le, Wd, P, D, X, case, lay):
    """wide_helpers.plan_heal for device.heal_ws: the totals and the
    workspace's tail beside it."""
    p = Wd.plan_heal(le, None, case, lay)
    p.kind = "heal_ws"
    masks = p.info["masks"]
    need = X.head(Wd.NOBJ)
    p.words_pre["totals"] = Wd._sentinels([X.TOTALS_PREFILL] * 2, P.SENTINELS)
    p.words_want["totals"] = Wd._sentinels([sum(1 for mk in masks if mk), 0], P.SENTINELS)
    p.words_want["workspace tail"] = Wd.WS_TAIL_WANT

    def run(gpu, le, arena, words):
        objs, par = Wd._views(arena, lay, case)
        lost, unhealed = Wd._i32(gpu, words["masks"]), Wd._i32(gpu, words["unhealed"])
        totals = Wd._i32(gpu, words["totals"])
        ws = Wd._workspace(gpu, need)
        le.device.heal_ws(case.cls, case.params, objs, case.size, par, lost,
                          unhealed=unhealed[1:1 + Wd.NOBJ], totals=totals[1:3], workspace=ws[:need])
        gpu.cuda.synchronize()
        return {"masks": D._u32(lost), "unhealed": D._u32(unhealed), "totals": D._u32(totals),
                "workspace tail": Wd._tail(ws, need)}
    p.run = run
    return p


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import heal_helpers as P
    import heal_ws_helpers as X
    import scrub_dev_helpers as D
    import wide_helpers as Wd

    oracle.lib()
    assert all(f in Wd.FAMILIES and not P.fused(*f[:4]) for f in FAMILIES)
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    try:
        arena = Wd.Arena(torch, Wd.arena_used(le))
    except RuntimeError as e:  # (torch's out-of-memory error is one)
        print(f"the wide allocation cannot be made: {str(e)[:200]}", flush=True)
        return 3
    failed = 0
    for family in FAMILIES:
        t0 = time.monotonic()
        p = plan_heal_ws(le, Wd, P, D, X, Wd.wide_case(le, oracle, family), Wd.layout(le, family))
        errors = Wd.execute(torch, le, arena, p)
        failed += bool(errors)
        print(json.dumps({"case": p.ident(), "errors": errors[:8],
                          "seconds": round(time.monotonic() - t0, 3)}), flush=True)
    print(json.dumps({"done": len(FAMILIES), "peak_bytes": torch.cuda.max_memory_allocated()}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
