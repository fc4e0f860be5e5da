"""gf8_heal_list<K> for every K = 1..16 in one fresh process: a plain script,
run by test_gf8_instances.py::test_gf8_heal_list_every_k_in_own_process.

leoec_scrub_dev rebuilds with gf8_heal_list only when the configuration has
one of heal.hip's at most 16 pattern tables, one per (class, k, m, device);
the 17th silently takes the composed path (leoec_locate_dev, then
leoec_heal_dev's other kernels).  So this process scrubs exactly 16
configurations, one per K, and nothing else:

  m = 2 + (K - 1) % 3 (scrub needs m >= 2), vandrs for odd K and isars for even K

Per configuration and size (4224 k - 3 and 128 (k - 1) + 5, the sizes of
test_gf8_instances.py) two calls through scrub_dev_helpers.SCRUB.check_scrub, every
byte against the oracle's snapshot: scrub_helpers' whole-block batch (every
valid byte of block b damaged in object b) and its position batch (64 values
at the block's first byte or in its last partial tile).  After each call the
workspace must hold scrub_finish's list (scrub_dev_helpers.path): the rebuild
was gf8_heal_list's.  Before any device call the script checks that it touches
no more than 16 configurations and, on the host, that leoec_heal_rows gives
every single-block mask a record (the configuration has a table).  Errors are
printed; the exit status is non-zero on any.

Usage: python tests/scrub_instances_child.py"""
import os
import sys

MAX_TABLES = 16  # heal.hip's kMaxHealTables
CONFIGS = [("vandrs" if k % 2 else "isars", k, 2 + (k - 1) % 3) for k in range(1, 17)]


def sizes(k):
    return [4224 * k - 3, 128 * (k - 1) + 5]


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import locate_helpers as L
    import scrub_dev_helpers as D
    import scrub_helpers as S

    oracle.lib()
    assert len(set(CONFIGS)) == len(CONFIGS) <= MAX_TABLES
    errors = []
    for cls, k, m in CONFIGS:
        for b in range(k + m):
            index = le.device.heal_rows(cls, (k, m, 8), 1 << b, coef=False)[3]
            if index < 0:
                errors.append(f"{cls}({k},{m}) mask {1 << b:#x}: no record (index {index})")
    if errors:
        print("\n".join(errors[:20]))
        return 1
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    touched = set()
    for cls, k, m in CONFIGS:
        touched.add((cls, k, m))
        assert len(touched) <= MAX_TABLES
        cfg = (cls, k, m, 8)
        for size in sizes(k):
            errs = []
            case = H.EdgeCase(le, oracle, cfg, size, k + m + 1)
            blocks = S.whole_batch(case)
            want = S.whole_words(case, blocks)
            assert all(want[b] == 1 << b for b in range(k + m))  # no empty block at these sizes
            batches = [("whole blocks", case, S.whole_arenas(torch, case, blocks), want, None)]
            case = H.EdgeCase(le, oracle, cfg, size, k + m + 2)
            dmg, _, locate = S.position_batch(case)
            want = S.two_block_word(oracle, le, case, dmg, locate)
            skip = None if want[-1] == S.MANY else case.n - 1
            assert skip is None or m == 2
            batches.append(("positions", case, L.damaged_arenas(torch, case, dmg), want, skip))
            for name, case, (work, par), want, skip in batches:
                keep = []
                report, es = D.SCRUB.check_scrub(torch, le, case, work, par, want, skip, keep=keep)
                errs += [f"{name}: {e}" for e in es]
                # (the report's own words: the object left out of the comparison is listed by its)
                path = D.path(torch, keep[0], D._u32(report)[1:-1])
                if path != "list":
                    errs.append(f"{name}: {case.ident()}: not the kernel path: {path}")
            errors += errs
            print(f"{cls}({k},{m}) size {size} bs {case.bs}: {2 * (k + m) + 3} objects, "
                  f"{len(errs)} errors", flush=True)
    if errors:
        print("\n".join(errors[:20]))
        return 1
    print(f"{len(touched)} configurations scrubbed")
    return 0


if __name__ == "__main__":
    sys.exit(main())
