"""gf8_heal<K> for every K = 1..16 in one fresh process: a plain script, run
by test_gf8_instances.py::test_gf8_heal_every_k_in_own_process.

heal.hip keeps at most 16 pattern tables per process, one per (class, k, m,
device); the 17th silently takes the generic path.  So this process heals
exactly 16 configurations, one per K, and nothing else:

  group a   m = 1 + (K-1) % 4, vandrs for odd K and isars for even K
  group b   m = 1 + (K+1) % 4, the classes swapped

Per configuration and size (4224 k - 3 and 128 (k-1) + 5, the sizes of
test_gf8_instances.py) one heal_helpers.run_heal over one object per mask: every
single block, the cyclic runs of 2..m blocks from every block, one clean
object and the two unrecoverable kinds.  Before any heal the script checks on
the host that leoec_heal_rows gives every recoverable mask a record (the
configuration has a table) and that it touches no more than 16
configurations.  Errors are printed; the exit status is non-zero on any.

Usage: python tests/gf8_heal_instances_child.py a|b"""
import os
import sys

MAX_TABLES = 16  # heal.hip's kMaxHealTables


def _group(shift, odd, even):
    return [(odd if k % 2 else even, k, 1 + (k + shift) % 4) for k in range(1, 17)]


GROUPS = {"a": _group(-1, "vandrs", "isars"), "b": _group(1, "isars", "vandrs")}


def sizes(k):
    return [4224 * k - 3, 128 * (k - 1) + 5]


def masks_of(k, m):
    """One mask per object: the k + m single blocks; for p = 2..m the cyclic
    runs {b, ..., b + p - 1 mod (k + m)} from every b; clean; m + 1 blocks and
    a bit at k + m (both unrecoverable)."""
    n = k + m
    out = [1 << b for b in range(n)]
    for p in range(2, m + 1):
        out += [sum(1 << ((b + x) % n) for x in range(p)) for b in range(n)]
    return out + [0, (1 << (m + 1)) - 1, 1 | 1 << n]


def main(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import gpu_helpers as H
    import heal_helpers as P

    oracle.lib()
    group = GROUPS[name]
    assert len(set(group)) <= MAX_TABLES
    errors = []
    # the host side first: every recoverable mask has a record
    for cls, k, m in group:
        masks = masks_of(k, m)
        assert all(a != b for a, b in zip(masks, masks[1:])), (cls, k, m)
        for mask in masks:
            if mask and P.recoverable(mask, k, m):
                index = le.device.heal_rows(cls, (k, m, 8), mask, coef=False)[3]
                if index < 0:
                    errors.append(f"{cls}({k},{m}) mask {mask:#x}: no record (index {index})")
    if errors:
        print("\n".join(errors[:20]))
        return 1
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    touched = set()
    for cls, k, m in group:
        touched.add((cls, k, m))
        assert len(touched) <= MAX_TABLES
        masks = masks_of(k, m)
        for size in sizes(k):
            case = H.EdgeCase(le, oracle, (cls, k, m, 8), size, len(masks))
            errs = P.run_heal(torch, le, case, masks)
            errors += errs
            print(f"{cls}({k},{m}) size {size} bs {case.bs}: {len(masks)} objects, "
                  f"{len(errs)} errors", flush=True)
    if errors:
        print("\n".join(errors[:20]))
        return 1
    print(f"group {name}: {len(touched)} configurations healed")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in GROUPS:
        sys.exit(__doc__.strip().splitlines()[-1])
    sys.exit(main(sys.argv[1]))
