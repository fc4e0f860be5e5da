"""leoec_heal_ws_dev with its table cache full, in one fresh process: a plain
script, run by test_device_heal_ws.py::
test_heal_ws_with_full_table_cache_in_own_process.

heal_ws.hip keeps at most 16 pattern tables per process, one per (class, k, m,
w, device).  This process first heals a batch of 3 objects under 16 small
vandrs w = 16 configurations (k = 2..9, m = 2 and 3), which fills the cache,
and then heals the edge-mask batch of a 17th, vandrs(10,4,16): the call finds
no table, writes unhealed and counts the totals with its listing kernel alone
and runs leoec_heal_dev's own path, and must leave every byte, unhealed and the
totals as the batch expects and as device.heal leaves them.  Which path a call
took shows in the workspace it leaves: with a table header word 0 holds the
number of listed objects, without one the header is untouched.  Errors are
printed; the exit status is non-zero on any.

Usage: python tests/heal_ws_table_cache_child.py"""
import os
import sys

MAX_TABLES = 16  # heal_ws.hip: DevTableCache<..., 16> of heal_ws_table
FILL = [("vandrs", k, m, 16) for m in (2, 3) for k in range(2, 10)]
LAST = ("vandrs", 10, 4, 16, 8704)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import heal_helpers as HH
    import heal_ws_helpers as X

    oracle.lib()
    assert len(set(FILL)) == MAX_TABLES and LAST[:4] not in FILL and LAST in HH.FAMILIES
    assert not any(HH.fused(*cfg) for cfg in FILL + [LAST[:4]])
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    errors = []
    fill_word = int.from_bytes(bytes([X.WS_FILL]) * 4, "little")

    def header_after(case, masks):
        work, par, _, _ = X.damaged(torch, case, masks)
        buf = X.Buffers(torch, masks)
        X.call(le, case, work, par, buf)
        torch.cuda.synchronize()
        return X.u32(buf.ws[:16].view(torch.int32))[0]

    for cfg in FILL:
        cls, k, m, w = cfg
        case = H.EdgeCase(le, oracle, cfg, 16 * k * w * 4 + 5, 3)
        masks = [HH.bits([0, k]), 0, HH.bits([k - 1])]
        errors += X.run_heal_ws(torch, le, case, masks)
    print(f"{len(FILL)} configurations healed, {len(errors)} errors", flush=True)
    # the 16th configuration has a table: the header holds the count
    count = header_after(case, masks)
    if count != 2:
        errors.append(f"{case.ident()}: the kernel path's header word {count:#x}, expected 2")
    cls, k, m, w, B = LAST
    for size in X.sizes(LAST)[:2]:
        case = H.edge_case(le, oracle, LAST[:4], size, n=HH.EDGE_N)
        masks = HH.edge_masks(k, m)
        errors += X.run_heal_ws(torch, le, case, masks)
        errors += X.run_heal_ws(torch, le, case, masks, nobj=HH.EDGE_N - 2)
        count = header_after(case, masks)
        if count != fill_word:
            errors.append(f"{case.ident()}: not the composed path's workspace: header word {count:#x}")
        print(f"{case.ident()} bs {case.bs}: {len(errors)} errors", flush=True)
    if errors:
        print("\n".join(e[:1500] for e in errors[:20]))
        return 1
    print("17th configuration healed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
