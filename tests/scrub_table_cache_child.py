"""leoec_scrub_dev, leoec_scrub_ws_dev or leoec_scrub_gfw_dev with the call's
table cache full, in one fresh process: a plain script, run by the
test_scrub*_with_full_table_cache_in_own_process tests of test_device_scrub.py,
test_device_scrub_ws.py and test_device_scrub_gfw.py.

The library keeps at most 16 tables per process for each call: heal.hip one
pattern table per (class, k, m, device), which scrub uses; scrub.hip one block
table per (class, k, m, w, device) for scrub_ws and one for scrub_gfw.  This
process first fills the call's cache with 16 small configurations (FILL: for
scrub one object healed under each, which fills heal's cache; for the other two
a scrub of 3 objects, one of them damaged) and then scrubs the position batch
and the dense batch of a 17th (LAST): the call finds no table, runs its locate
and leoec_heal_dev's other path, and must leave the report, the totals and
every byte as the call's locate + device.heal leave them, and as the batches
expect by construction.  Which path a call took shows in the workspace it
leaves (scrub_dev_helpers.path): the kernel path zeroes the header and writes
the list (word 0 the count, the index words a permutation of the named
objects), the composed path leaves the header as it found it and fills the
index words with leoec_heal_dev's `unhealed`, all zero on a batch in which
every object names a block.  The dense batch is looked at that way under the
16th configuration (a table: the list) and under the 17th (none: zeros).
Errors are printed; the exit status is non-zero on any.

Usage: python tests/scrub_table_cache_child.py scrub|scrub_ws|scrub_gfw"""
import os
import sys

MAX_TABLES = 16  # heal.hip's kMaxHealTables; scrub.hip's DevTableCache<..., 16> of both block tables
# call: (the 16 configurations, the 17th, bytes of a data block of a fill case)
CALLS = {
    "scrub": ([(cls, k, 2, 8) for cls in ("vandrs", "isars") for k in range(1, 9)],
              ("vandrs", 10, 4, 8, 8704), 128),
    "scrub_ws": ([("cauchyrs", k, m, 4) for m in (2, 3) for k in range(2, 10)],
                 ("cauchyrs", 10, 4, 8, 4352 * 8), 64 * 4),
    "scrub_gfw": ([("vandrs", k, m, 16) for m in (2, 3) for k in range(2, 10)],
                  ("vandrs", 10, 4, 16, 8704), 16 * 16 * 4),
}


def workspace_after(torch, le, D, L, X, case):
    """One call over the case's dense batch and a workspace of WS_FILL bytes:
    (header word 0, the n index words) as the call leaves them."""
    n, g = case.n, case.guard
    dmg, want = D.dense_batch(case)
    assert all(x not in (0, L.MANY) for x in want), want  # every object names a block
    work, par = L.damaged_arenas(torch, case, dmg)
    need = X.workspace_bytes(le, case)
    ws = torch.full((need,), D.WS_FILL, dtype=torch.uint8, device="cuda")
    report, totals = getattr(le.device, X.name)(case.cls, case.params, work[g:g + n], case.size,
                                                par[1:1 + n], workspace=ws)
    torch.cuda.synchronize()
    assert D._u32(report) == want and totals.tolist() == [n, 0], (D._u32(report), totals.tolist())
    words = D._u32(ws[:16 + 4 * n].view(torch.int32))
    return words[0], words[4:4 + n]


def main(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import heal_helpers as P
    import locate_gfw_helpers as G
    import locate_helpers as L
    import locate_ws_helpers as W
    import scrub_dev_helpers as D
    import scrub_helpers as S

    oracle.lib()
    X = {x.name: x for x in D.CALLS}[name]
    FILL, LAST, B = CALLS[name]
    assert len(set(FILL)) == MAX_TABLES and LAST[:4] not in FILL and LAST in X.FAMILIES
    # every one is of the call's own classes, not one it forwards
    own = {"scrub": L.served, "scrub_ws": lambda *c: W.served(*c) and not L.served(*c),
           "scrub_gfw": G.word_class}[name]
    assert all(own(*cfg) for cfg in FILL + [LAST[:4]])
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    errors = []
    for cfg in FILL:
        cls, k, m, w = cfg
        if name == "scrub":
            # every one has a record table (the cache counts only those)
            assert le.device.heal_rows(cls, (k, m, w), 1, coef=False)[3] >= 0, cfg
            case = H.EdgeCase(le, oracle, cfg, B * k + 5, 1)
            errors += P.run_heal(torch, le, case, [1])
        else:
            case = H.EdgeCase(le, oracle, cfg, B * k + 5, 3)
            dmg = S._entries(case, 1, 0, S.VALUES[:S.HITS])
            work, par = L.damaged_arenas(torch, case, dmg)
            errors += X.check_scrub(torch, le, case, work, par, [0, 1, 0])[1]
    print(f"{len(FILL)} configurations filled, {len(errors)} errors", flush=True)
    fill_word = int.from_bytes(bytes([D.WS_FILL]) * 4, "little")
    # the 16th configuration has a table: the header holds the count, the index words the list
    cls, k, m, w = FILL[-1]
    case = H.EdgeCase(le, oracle, FILL[-1], B * k, k + m)  # every block whole: every object named
    count, index = workspace_after(torch, le, D, L, X, case)
    if count != case.n or sorted(index) != list(range(case.n)):
        errors.append(f"{case.ident()}: the kernel path's workspace: count {count}, list {index}")
    for case in X.cases(le, oracle, LAST, D.sizes(LAST)):
        dmg, want, skip = X.position(le, oracle, case)
        work, par = L.damaged_arenas(torch, case, dmg)
        errors += X.check_scrub(torch, le, case, work, par, want, skip)[1]
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
    sys.exit(main(sys.argv[1]))
