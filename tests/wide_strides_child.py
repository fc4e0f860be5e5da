"""The heal, scrub and scrub_ws cases of test_device_wide_strides.py in one
fresh process: a plain script, run by
test_device_wide_strides.py::test_heal_and_scrub_in_own_process.

leoec_heal_dev and leoec_scrub_dev serve the fused GF(2^8) configurations from
heal.hip's at most 16 pattern tables, leoec_scrub_ws_dev the bitmatrix classes
from its own at most 16 block tables; a configuration past the 16th silently
takes the composed path.  Which kernel serves a call therefore depends on what
ran before it in the process, so this process runs these cases and nothing
else: 4 pattern tables and 6 block tables.  Before any device call the script
checks those counts and, on the host, that leoec_heal_rows gives every mask a
fused configuration is healed with a record (gf8_heal reads the table).  After
each scrub call the workspace must hold scrub_finish's list
(scrub_dev_helpers.path): the rebuild was gf8_heal_list's or bit_heal_list's.

The batches are wide_helpers' plans: three objects whose rows lie 2^32 + 48
bytes apart in one device allocation of this process's own.  One JSON line per
case ({"case", "errors", "path", "seconds"}) and a last one with the process's
peak device memory; the parent asserts on them.  The first exception ends the
script: nothing more is started on the device after a failed call.

Usage: python tests/wide_strides_child.py"""
import json
import os
import sys
import time

MAX_TABLES = 16  # heal.hip's kMaxHealTables, scrub_bit_table.cpp's cache


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import torch

    import leo_erasure_amd as le
    from oracle import oracle

    import heal_helpers as P
    import wide_helpers as Wd

    oracle.lib()
    todo = [(f, kind, var) for f in Wd.FAMILIES for kind, var in Wd.calls(f) if kind in Wd.CHILD_KINDS]
    pattern = {f[:3] for f, kind, _ in todo if P.fused(*f[:4])}
    block = {f[:4] for f, kind, _ in todo if kind == "scrub_ws"}
    assert 0 < len(pattern) <= MAX_TABLES and 0 < len(block) <= MAX_TABLES, (pattern, block)
    for f in Wd.FAMILIES:
        if P.fused(*f[:4]):
            case = Wd.wide_case(le, oracle, f)
            for mask in Wd.heal_masks(case) + [1 << b for b in Wd.locate_blocks(case) if b is not None]:
                if mask:
                    index = le.device.heal_rows(f[0], f[1:4], mask, coef=False)[3]
                    assert index >= 0, (f, hex(mask), index)
    assert torch.cuda.is_available(), "needs a HIP device"
    assert le.gf_init() == "ok", le.gf_init()
    arena = Wd.Arena(torch, Wd.arena_used(le))
    for family, kind, var in todo:
        t0 = time.monotonic()
        p = Wd.plan(le, oracle, family, kind, var)
        errors = Wd.execute(torch, le, arena, p)
        path = p.info.get("path")
        if kind != "heal" and path != "list":
            errors.append(f"{p.ident()}: not the kernel path: {path}")
        print(json.dumps({"case": p.ident(), "errors": errors[:8], "path": path,
                          "seconds": round(time.monotonic() - t0, 3)}), flush=True)
    print(json.dumps({"done": len(todo), "peak_bytes": torch.cuda.max_memory_allocated(),
                      "pattern_tables": len(pattern), "block_tables": len(block)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
