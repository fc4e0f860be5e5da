"""leoec_scrub_dev with heal's table cache full, in one fresh process: a plain
script, run by test_device_scrub.py::
test_scrub_with_full_table_cache_in_own_process.

heal.hip keeps at most 16 pattern tables per process, one per (class, k, m,
device).  This process first heals one object under 16 small configurations
(vandrs and isars, k = 1..8, m = 2), which fills the cache, and then scrubs the
position batch and the dense batch of a 17th, vandrs(10,4,8): the call finds
no table, runs leoec_locate_dev and leoec_heal_dev's other path, and must
leave the report, the totals and every byte as device.locate + device.heal
leave them, and as the batches expect by construction.  Errors are printed;
the exit status is non-zero on any.

Usage: python tests/scrub_table_cache_child.py"""
import os
import sys

MAX_TABLES = 16  # heal.hip's kMaxHealTables
FILL = [(cls, k, 2) for cls in ("vandrs", "isars") for k in range(1, 9)]
LAST = ("vandrs", 10, 4, 8, 8704)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import heal_helpers as P
    import locate_helpers as L
    import scrub_dev_helpers as D
    import scrub_helpers as S

    oracle.lib()
    assert len(set(FILL)) == MAX_TABLES and LAST[:3] not in FILL
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    errors = []
    for cls, k, m in FILL:
        # every one has a record table (the cache counts only those)
        assert le.device.heal_rows(cls, (k, m, 8), 1, coef=False)[3] >= 0, (cls, k, m)
        case = H.EdgeCase(le, oracle, (cls, k, m, 8), 128 * k + 5, 1)
        errors += P.run_heal(torch, le, case, [1])
    print(f"{len(FILL)} configurations healed, {len(errors)} errors", flush=True)
    for case in D.position_cases(le, oracle, LAST):
        dmg, _, locate = S.position_batch(case)
        want = S.two_block_word(oracle, le, case, dmg, locate)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += D.check_scrub(torch, le, case, work, par, want)[1]
        errors += D.check_equivalence(torch, le, case, dmg)[3]
        dmg, want = D.dense_batch(case)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += D.check_scrub(torch, le, case, work, par, want)[1]
        errors += D.check_equivalence(torch, le, case, dmg)[3]
        print(f"{case.ident()} bs {case.bs}: {len(errors)} errors", flush=True)
    if errors:
        print("\n".join(errors[:20]))
        return 1
    print("17th configuration scrubbed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
