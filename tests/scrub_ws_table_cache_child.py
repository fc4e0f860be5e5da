"""leoec_scrub_ws_dev with its block table cache full, in one fresh process: a
plain script, run by test_device_scrub_ws.py::
test_scrub_ws_with_full_table_cache_in_own_process.

scrub.hip keeps at most 16 block tables per process, one per (class, k, m, w,
device).  This process first scrubs a batch of 3 objects, one of them damaged,
under 16 small cauchyrs configurations (k = 2..9, m = 2 and 3, w = 4), which
fills the cache, and then scrubs the position batch and the dense batch of a
17th, cauchyrs(10,4,8): the call finds no table, runs leoec_locate_ws_dev and
leoec_heal_dev's other path, and must leave the report, the totals and every
byte as device.locate_ws + device.heal leave them, and as the batches expect
by construction.  Which path a call took shows in the workspace it leaves: the
kernel path zeroes the header and writes the list (word 0 the count, the index
words a permutation of the named objects), the composed path leaves the header
as it found it and fills the index words with leoec_heal_dev's `unhealed`, all
zero on a batch in which every object names a block.  The dense batch is
looked at that way under the 16th configuration (a table: the list) and under
the 17th (none: zeros).  Errors are printed; the exit status is non-zero on any.

Usage: python tests/scrub_ws_table_cache_child.py"""
import os
import sys

MAX_TABLES = 16  # scrub.hip's kMaxScrubBitTables
FILL = [("cauchyrs", k, m, 4) for m in (2, 3) for k in range(2, 10)]
LAST = ("cauchyrs", 10, 4, 8, 4352 * 8)


def workspace_after(torch, le, D, L, X, case):
    """One scrub_ws of the case's dense batch over a workspace of 0x6B bytes:
    (header word 0, the n index words) as the call leaves them."""
    n, g = case.n, case.guard
    dmg, want = D.dense_batch(case)
    assert all(x not in (0, L.MANY) for x in want), want  # every object names a block
    work, par = L.damaged_arenas(torch, case, dmg)
    need = X.workspace_bytes(le, case)
    ws = torch.full((need,), X.WS_FILL, dtype=torch.uint8, device="cuda")
    report, totals = le.device.scrub_ws(case.cls, case.params, work[g:g + n], case.size,
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
    import locate_helpers as L
    import locate_ws_helpers as W
    import scrub_dev_helpers as D
    import scrub_helpers as S
    import scrub_ws_helpers as X

    oracle.lib()
    assert len(set(FILL)) == MAX_TABLES and LAST[:4] not in FILL and LAST in W.FAMILIES
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    errors = []
    for cfg in FILL:
        cls, k, m, w = cfg
        case = H.EdgeCase(le, oracle, cfg, 64 * k * w + 5, 3)
        dmg = S._entries(case, 1, 0, S.VALUES[:S.HITS])
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, [0, 1, 0])[1]
    print(f"{len(FILL)} configurations scrubbed, {len(errors)} errors", flush=True)
    fill_word = int.from_bytes(bytes([X.WS_FILL]) * 4, "little")
    # the 16th configuration has a table: the header holds the count, the index words the list
    cls, k, m, w = FILL[-1]
    case = H.EdgeCase(le, oracle, FILL[-1], 64 * k * w, k + m)  # every block whole: every object named
    count, index = workspace_after(torch, le, D, L, X, case)
    if count != case.n or sorted(index) != list(range(case.n)):
        errors.append(f"{case.ident()}: the kernel path's workspace: count {count}, list {index}")
    for case in D.position_cases(le, oracle, LAST):
        dmg, _, locate = S.position_batch(case)
        want = S.two_block_word(oracle, le, case, dmg, locate)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, want)[1]
        errors += X.check_equivalence(torch, le, case, dmg)[4]
        dmg, want = D.dense_batch(case)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, want)[1]
        errors += X.check_equivalence(torch, le, case, dmg)[4]
        if case.size == D.sizes(LAST)[0]:
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
