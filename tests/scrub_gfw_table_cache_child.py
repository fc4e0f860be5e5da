"""leoec_scrub_gfw_dev with its block table cache full, in one fresh process: a
plain script, run by test_device_scrub_gfw.py::
test_scrub_gfw_with_full_table_cache_in_own_process.

scrub.hip keeps at most 16 word block tables per process, one per (class, k,
m, w, device).  This process first scrubs a batch of 3 objects, one of them
damaged, under 16 small vandrs w = 16 configurations (k = 2..9, m = 2 and 3),
which fills the cache, and then scrubs the position batch and the dense batch
of a 17th, vandrs(10,4,16): the call finds no table, runs leoec_locate_gfw_dev
and leoec_heal_dev's other path, and must leave the report, the totals and
every byte as device.locate_gfw + device.heal leave them, and as the batches
expect by construction.  Which path a call took shows in the workspace it
leaves (scrub_dev_helpers.path): the dense batch is looked at that way under
the 16th configuration (a table: the list) and under the 17th (none: the
header untouched, heal's `unhealed` zeros in the index words).  Errors are
printed; the exit status is non-zero on any.

Usage: python tests/scrub_gfw_table_cache_child.py"""
import os
import sys

MAX_TABLES = 16  # scrub.hip: DevTableCache<..., 16> of scrub_gfw_table
FILL = [("vandrs", k, m, 16) for m in (2, 3) for k in range(2, 10)]
LAST = ("vandrs", 10, 4, 16, 8704)


def workspace_after(torch, le, D, L, X, case):
    """One scrub_gfw of the case's dense batch over a workspace of 0x6B bytes:
    (header word 0, the n index words) as the call leaves them."""
    n, g = case.n, case.guard
    dmg, want = D.dense_batch(case)
    assert all(x not in (0, L.MANY) for x in want), want  # every object names a block
    work, par = L.damaged_arenas(torch, case, dmg)
    need = X.workspace_bytes(le, case)
    ws = torch.full((need,), X.WS_FILL, dtype=torch.uint8, device="cuda")
    report, totals = le.device.scrub_gfw(case.cls, case.params, work[g:g + n], case.size,
                                         par[1:1 + n], workspace=ws)
    torch.cuda.synchronize()
    assert D._u32(report) == want and totals.tolist() == [n, 0], (D._u32(report), totals.tolist())
    words = D._u32(ws[:16 + 4 * n].view(torch.int32))
    return words[0], words[4:4 + n]


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import locate_gfw_helpers as G
    import locate_helpers as L
    import scrub_dev_helpers as D
    import scrub_gfw_helpers as X
    import scrub_helpers as S

    oracle.lib()
    assert len(set(FILL)) == MAX_TABLES and LAST[:4] not in FILL and LAST in G.FAMILIES
    assert all(G.word_class(*cfg) for cfg in FILL)
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    errors = []
    for cfg in FILL:
        cls, k, m, w = cfg
        case = H.EdgeCase(le, oracle, cfg, 16 * k * w * 4 + 5, 3)
        dmg = S._entries(case, 1, 0, S.VALUES[:S.HITS])
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, [0, 1, 0])[1]
    print(f"{len(FILL)} configurations scrubbed, {len(errors)} errors", flush=True)
    fill_word = int.from_bytes(bytes([X.WS_FILL]) * 4, "little")
    # the 16th configuration has a table: the header holds the count, the index words the list
    cls, k, m, w = FILL[-1]
    case = H.EdgeCase(le, oracle, FILL[-1], 16 * k * w * 4, k + m)  # every block whole: every object named
    count, index = workspace_after(torch, le, D, L, X, case)
    if count != case.n or sorted(index) != list(range(case.n)):
        errors.append(f"{case.ident()}: the kernel path's workspace: count {count}, list {index}")
    for case in X.cases(le, oracle, LAST, X.sizes(LAST)[:2]):
        dmg, want, skip = X.position(le, oracle, case)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, want, skip)[1]
        errors += X.check_equivalence(torch, le, case, dmg)[4]
        dmg, want = D.dense_batch(case)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, want)[1]
        errors += X.check_equivalence(torch, le, case, dmg)[4]
        if case.size == X.sizes(LAST)[0]:
            # no table for the 17th: the header untouched, the index words heal's unhealed
            count, index = workspace_after(torch, le, D, L, X, case)
            if count != fill_word or index != [0] * case.n:
                errors.append(f"{case.ident()}: not the composed path's workspace: header word "
                              f"{count:#x}, index words {index}")
        print(f"{case.ident()} bs {case.bs}: {len(errors)} errors", flush=True)
    if errors:
        print("\n".join(errors[:20]))
        return 1
    print("17th configuration scrubbed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
