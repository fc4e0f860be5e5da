"""gfw_heal_list<W>, the rebuild kernel of leoec_scrub_gfw_dev's word classes
(CPU test, on the objects build() leaves in leo_erasure_amd/csrc/_build and
_build_measure).

Three instances, W = 8, 16 and 32, with k and m runtime values, in both
libraries.  A lane holds one accumulator row and two input buffers of 16
registers each beside the multiply's temporaries: no instance may spill a
register or use scratch (a spilling kernel's first launch makes the runtime
back the whole device's scratch, test_code_objects.py), and each must fit the
4-wave register budget its fixed grid counts on (gfw_heal_list_resident: 16
workgroups a compute unit).  No LDS; one wave per workgroup; the table is in
memory, so the argument segment is what gfw_heal_tile.hpp asserts.  Metadata
only, read as test_locate_ws_code_object.py reads it."""
import os
import re

import pytest

import scrub_dev_helpers as D
import test_locate_ws_code_object as CO

X = D.SCRUB_GFW

CSRC = os.path.join(CO.ROOT, "leo_erasure_amd", "csrc")
OBJS = {"product": os.path.join(CSRC, "_build", "scrub.o"),
        "measure": os.path.join(CSRC, "_build_measure", "scrub.o")}
SRC = os.path.join(CSRC, "gfw_heal_tile.hpp")  # the constants, GfwHealArgs and resident()
NAME = "_ZN5leoec6detail13gfw_heal_listILi%dEEEvNS0_11GfwHealArgsEPKjS4_"


def _source():
    with open(SRC) as f:
        return f.read()


def asserted_argument_bytes():
    """The explicit argument bytes the source's static_assert states."""
    m = re.search(r"static_assert\(sizeof\(GfwHealArgs\) \+ 2 \* sizeof\(uint32_t\*\) == (\d+),", _source())
    assert m, "gfw_heal_tile.hpp: the argument segment's static_assert"
    return int(m.group(1))


def test_asserted_argument_segment():
    """HealArgs (eight 64-bit words, seven 32-bit ones, padded to 96 bytes),
    two more words, then the list and its count."""
    assert asserted_argument_bytes() == 8 * 8 + 8 * 4 + 2 * 4 + 2 * 8 == 120


def test_geometry_constants_are_the_sources():
    """The tile and the grid rule the device tests restate."""
    text = _source()
    assert re.findall(r"constexpr int kGfwHealLanes = (\d+);", text) == ["64"]
    assert "constexpr int kGfwHealLoads = gfwheal::kRegs / 4;" in text
    assert "constexpr uint32_t kGfwHealTile = kGfwHealLanes * 16u * kGfwHealLoads;" in text
    assert X.TILE == 64 * 16 * (16 // 4)
    assert re.findall(r"constexpr int kGfwHealWaves = (\d+);", text) == ["4"]
    assert "inline uint32_t gfw_heal_list_resident() { return 4u * (uint32_t)kGfwHealWaves; }" in text
    assert X.resident() == 4 * 4
    # the grid rule: the launcher hands its items and resident() to list_grid
    with open(os.path.join(CSRC, "scrub_gfw_impl.hpp")) as f:
        assert ("const dim3 g(list_grid((uint64_t)a.h.nobj * a.h.tiles, gfw_heal_list_resident(), cap));"
                in f.read())
    with open(os.path.join(CSRC, "heal_impl.hpp")) as f:
        heal = f.read()
    assert "uint64_t grid = (uint64_t)device_cus() * resident;" in heal
    assert "grid = grid < all ? grid : all;" in heal
    assert "if (cap != 0u && grid > cap) grid = cap;" in heal
    assert X.grid(256, 10, 3) == 30 and X.grid(256, 2048, 3) == 4096 and X.grid(256, 2048, 3, 7) == 7


@pytest.mark.parametrize("build", sorted(OBJS))
@pytest.mark.skipif(not all(os.path.exists(p) for p in OBJS.values()), reason="objects not built")
@pytest.mark.skipif(not all(CO._tool(t) for t in CO.TOOLS), reason="ROCm LLVM tools absent")
def test_gfw_heal_list_instances(tmp_path, build):
    notes = CO.kernel_notes(OBJS[build], str(tmp_path))
    found = {name: md for name, md in notes if "gfw_heal_list" in name and name.startswith("_Z")}
    assert sorted(found) == sorted(NAME % w for w in (8, 16, 32)), sorted(found)
    explicit = asserted_argument_bytes()
    for name, md in found.items():
        assert int(md["vgpr_spill_count"]) == 0, (name, md)
        assert int(md.get("sgpr_spill_count", "0")) == 0, (name, md)
        assert int(md.get("private_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md.get("group_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md["wavefront_size"]) == 64, (name, md)
        assert int(md["max_flat_workgroup_size"]) == 64, (name, md)
        # 4 waves per SIMD: at most 128 VGPRs (and no AGPRs)
        assert int(md["vgpr_count"]) <= 128, (name, md)
        assert int(md.get("agpr_count", "0")) == 0, (name, md)
        # the explicit arguments, and at most the hidden ones behind them
        assert explicit <= int(md["kernarg_segment_size"]) <= explicit + 256, (name, md)
    # the other two list kernels are still the instances their own tests expect
    assert len([n for n, _ in notes if "bit_heal_list" in n and n.startswith("_Z")]) == 1
    assert len([n for n, _ in notes if "scrub_finish" in n and n.startswith("_Z")]) == 1
