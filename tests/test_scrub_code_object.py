"""The kernels of leoec_scrub_dev (CPU test, on the objects build() leaves in
leo_erasure_amd/csrc/_build).

gf8_heal_list<K, 4> is gf8_heal's tile body inside a loop over a list, under
gf8_heal's 4-wave register budget: for every K = 1..16 it must spill no VGPR
and use no scratch, within 128 VGPRs, as test_code_objects.py asks of
gf8_heal (a spilling kernel's first launch makes the runtime back the whole
device's scratch).  scrub_finish, the compaction kernel, likewise.  The
metadata is read with test_code_objects.py's reader."""
import glob
import os

import pytest

from test_code_objects import BUILD, _tool, kernel_notes

TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
needs_objects = pytest.mark.skipif(not glob.glob(os.path.join(BUILD, "*.o")),
                                   reason="product objects not built")
needs_tools = pytest.mark.skipif(not all(_tool(t) for t in TOOLS), reason="ROCm LLVM tools absent")
HEAL_LIST = "_ZN5leoec6detail13gf8_heal_listILi%dELi4ELi4EEE"  # <K, R = 4, 4 waves>


@needs_objects
@needs_tools
def test_gf8_heal_list_does_not_spill(tmp_path):
    found = {}
    for K in range(1, 17):
        obj = os.path.join(BUILD, "gf8_scrub_k%d.o" % K)
        assert os.path.exists(obj), obj
        for name, md in kernel_notes(obj, str(tmp_path)):
            if name.startswith(HEAL_LIST % K):
                found[K] = (int(md["vgpr_spill_count"]), int(md.get("private_segment_fixed_size", "0")),
                            int(md.get("sgpr_spill_count", "0")), int(md["vgpr_count"]))
    assert sorted(found) == list(range(1, 17)), sorted(found)
    assert all(v[:2] == (0, 0) for v in found.values()), found
    # the 4-wave budget: at most 128 VGPRs
    assert max(v[3] for v in found.values()) <= 128, found


@needs_objects
@needs_tools
def test_scrub_finish_does_not_spill(tmp_path):
    obj = os.path.join(BUILD, "scrub.o")
    assert os.path.exists(obj), obj
    found = [(name, md) for name, md in kernel_notes(obj, str(tmp_path))
             if "scrub_finish" in name and name.startswith("_Z") and "vgpr_spill_count" in md]
    assert len(found) == 1, [name for name, _ in found]
    md = found[0][1]
    assert int(md["vgpr_spill_count"]) == 0, md
    assert int(md.get("sgpr_spill_count", "0")) == 0, md
    assert int(md.get("private_segment_fixed_size", "0")) == 0, md
