"""The kernels of leoec_heal_ws_dev (CPU test, on the objects build() leaves in
leo_erasure_amd/csrc/_build and _build_measure): heal_ws_begin, heal_ws_list,
gfw_heal_masks<8|16|32> and bit_heal_masks, in both libraries.

No instance may spill a register or use scratch, gfw_heal_masks must fit the
4-wave register budget its fixed grid counts on and use no LDS,
bit_heal_masks keeps its accumulators in dynamic LDS (no static LDS), and
heal_ws.o holds no second copy of a kernel that another unit defines
(gfw_heal_list, bit_heal_list, scrub_finish).  Metadata only, read as
test_locate_ws_code_object.py reads it."""
import os

import pytest

import test_locate_ws_code_object as CO

CSRC = os.path.join(CO.ROOT, "leo_erasure_amd", "csrc")
OBJS = {"product": os.path.join(CSRC, "_build", "heal_ws.o"),
        "measure": os.path.join(CSRC, "_build_measure", "heal_ws.o")}
GFW = "_ZN5leoec6detail14gfw_heal_masksILi%dEEEvNS0_11GfwHealArgsEPKjS4_"
WANT = sorted([GFW % w for w in (8, 16, 32)] +
              ["_ZN5leoec6detail14bit_heal_masksENS0_11BitHealArgsEPKjS3_",
               "_ZN5leoec6detail12heal_ws_listEPKjPjjjjS3_S3_S3_",
               "_ZN5leoec6detail13heal_ws_beginEPjS1_"])


@pytest.mark.parametrize("build", sorted(OBJS))
@pytest.mark.skipif(not all(os.path.exists(p) for p in OBJS.values()), reason="objects not built")
@pytest.mark.skipif(not all(CO._tool(t) for t in CO.TOOLS), reason="ROCm LLVM tools absent")
def test_heal_ws_kernels(tmp_path, build):
    found = {name: md for name, md in CO.kernel_notes(OBJS[build], str(tmp_path)) if name.startswith("_Z")}
    assert sorted(found) == WANT, sorted(found)
    for name, md in found.items():
        assert int(md["vgpr_spill_count"]) == 0, (name, md)
        assert int(md.get("sgpr_spill_count", "0")) == 0, (name, md)
        assert int(md.get("private_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md.get("group_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md.get("agpr_count", "0")) == 0, (name, md)
        assert int(md["wavefront_size"]) == 64, (name, md)
        if "heal_masks" in name:
            assert int(md["max_flat_workgroup_size"]) == 64, (name, md)
        if "gfw_heal_masks" in name:  # 4 waves per SIMD: at most 128 VGPRs
            assert int(md["vgpr_count"]) <= 128, (name, md)
