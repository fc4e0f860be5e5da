"""bit_heal_list across its runtime parameters in fresh processes: a plain
script, run by test_kernel_instances.py::
test_bit_heal_list_sweep_in_own_processes.

bit_heal_list (scrub_bit_impl.hpp) is one instance that takes w, k and m as
values.  leoec_scrub_ws_dev rebuilds with it only when the configuration has
one of scrub.hip's at most 16 block tables, one per (class, k, m, w, device);
the 17th silently takes the composed path (leoec_locate_ws_dev, then
leoec_heal_dev's kernels).  So each process scrubs one group of at most 16
configurations and nothing else.  Together the groups hold

  cauchyrs    every w = 2..32, m rotating over 2, 3, 4 (w <= 16) and over 3, 4
              above (both sides build an m = 2 Cauchy matrix from a sorted
              table of all 2^w elements and refuse it past w = 20; at w = 2
              only m = 2 leaves a k), k = 2 + w mod 5 as far as k + m <= 2^w
              and (m - 1) k w <= 768 allow; w = 8 and w = 32 are limits below;
  liberation  w = 3, 5, 7, 11, 13, 17, 19, 23, 29, 31 (k = min(w, 2 + w mod 5);
              w = 31 is a limit below);
  the limits  cauchyrs(27,4,8) and (29,2,8): k + m = 31, `word >> (k + m)` at
              31, 29 survivor ids in all 8 id words; cauchyrs(12,3,32): 768
              row words, a mask word with bit 31, 32 KiB of dynamic LDS;
              cauchyrs(6,4,32); liberation(24,2,31);
  k = 1       cauchyrs(1,2,8) and liberation(1,2,3): `vlast` is block 0's own
              valid length.

Two sizes each: k B - 1 with B = 1,040 w (one whole 1 KiB tile and a 16-byte
partial one per packet, the last block one byte short) and, for k >= 2,
16 w (k - 1) + 5 (packets of 16 bytes: a single tile with 63 lanes outside the
packet, the last block 5 bytes).  Per configuration and size two calls through
scrub_dev_helpers.SCRUB_WS.check_scrub, every byte against the oracle's snapshot:
scrub_helpers' whole-block batch (every valid byte of block b damaged in object
b) and its position batch.  After each call the workspace must hold
scrub_finish's list (scrub_dev_helpers.path): the rebuild was bit_heal_list's.
Before any device call the script checks that the group touches no more than
16 configurations.  Errors are printed; the exit status is non-zero on any.

Usage: python tests/scrub_ws_instances_child.py a|b|c"""
import os
import sys

MAX_TABLES = 16  # scrub.hip's kMaxScrubBitTables
MAX_WORDS = 768  # (m - 1) k w at most
LIB_WS = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31)
LIMITS = [("cauchyrs", 27, 4, 8), ("cauchyrs", 29, 2, 8), ("cauchyrs", 12, 3, 32),
          ("cauchyrs", 6, 4, 32), ("liberation", 24, 2, 31)]
ONES = [("cauchyrs", 1, 2, 8), ("liberation", 1, 2, 3)]
PACKET = 1040  # bytes of a packet at the first size: a 1 KiB tile and 16 bytes


def cauchy_config(w):
    if w == 2:
        return ("cauchyrs", 2, 2, 2)
    m = (2, 3, 4)[w % 3] if w <= 16 else (3, 4)[w % 2]
    k = min(2 + w % 5, (1 << w) - m, MAX_WORDS // ((m - 1) * w), 31 - m)
    return ("cauchyrs", k, m, w)


def liberation_config(w):
    return ("liberation", min(w, 2 + w % 5, MAX_WORDS // w), 2, w)


def configs():
    """Every configuration once: the two sweeps with the limits of w = 8, 32
    and 31 in their places, then the remaining limits and k = 1."""
    at = {("cauchyrs", 8): LIMITS[0], ("cauchyrs", 32): LIMITS[2], ("liberation", 31): LIMITS[4]}
    out = [at.get(("cauchyrs", w), cauchy_config(w)) for w in range(2, 33)]
    out += [at.get(("liberation", w), liberation_config(w)) for w in LIB_WS]
    out += [c for c in LIMITS + ONES if c not in out]
    return out


# dealt in turn, so that each group has its share of the wide ones
GROUPS = {name: configs()[i::3] for i, name in enumerate("abc")}


def sizes(cfg):
    cls, k, m, w = cfg
    return [k * PACKET * w - 1] + ([16 * w * (k - 1) + 5] if k >= 2 else [])


def main(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import locate_helpers as L
    import scrub_dev_helpers as D
    X = D.SCRUB_WS
    import scrub_helpers as S

    oracle.lib()
    group = GROUPS[name]
    assert len(set(group)) == len(group) <= MAX_TABLES
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    errors = []
    touched = set()
    for cfg in group:
        touched.add(cfg)
        assert len(touched) <= MAX_TABLES
        cls, k, m, w = cfg
        for size in sizes(cfg):
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
            for what, case, (work, par), want, skip in batches:
                keep = []
                report, es = X.check_scrub(torch, le, case, work, par, want, skip, keep=keep)
                errs += [f"{what}: {e}" for e in es]
                # (the report's own words: the object left out of the comparison is listed by its)
                path = D.path(torch, keep[0], D._u32(report)[1:-1])
                if path != "list":
                    errs.append(f"{what}: {case.ident()}: not the kernel path: {path}")
            errors += errs
            print(f"{cls}({k},{m},{w}) size {size} bs {case.bs}: {2 * (k + m) + 3} objects, "
                  f"{len(errs)} errors", flush=True)
    if errors:
        print("\n".join(errors[:20]))
        return 1
    print(f"group {name}: {len(touched)} configurations scrubbed")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in GROUPS:
        sys.exit(__doc__.strip().splitlines()[-1])
    sys.exit(main(sys.argv[1]))
