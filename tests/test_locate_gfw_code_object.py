"""gfw_locate<W>, the kernel behind leoec_locate_gfw_dev's word classes (CPU
test, on the objects build() leaves in leo_erasure_amd/csrc/_build).

Three instances, W = 8, 16 and 32, with k and m runtime values.  The dirty
path multiplies a syndrome of 16 registers by up to 240 ratios with the
bitsliced multiply of gfs_core.hpp; no instance may spill a register or use
scratch (a spilling kernel's first launch makes the runtime back the whole
device's scratch, test_code_objects.py), and the clean path, which is all a
clean batch runs, must not pay for the dirty one in waves per SIMD: s_0 waits
in 4 KiB of LDS and every instance fits the 8-wave register budget.  The ratio
table is a kernel argument: the argument segment is what locate_gfw_impl.hpp
asserts.  The metadata is read as test_locate_ws_code_object.py reads it."""
import os
import re

import pytest

import test_locate_ws_code_object as CO

OBJ = CO.OBJ
SRC = os.path.join(CO.ROOT, "leo_erasure_amd", "csrc", "locate_gfw_impl.hpp")
NAME = "_ZN5leoec6detail10gfw_locateILi%dEEEvNS0_10GfwLocArgsEPj"


def asserted_argument_bytes():
    """The explicit argument bytes the source's static_assert states."""
    with open(SRC) as f:
        m = re.search(r"static_assert\(sizeof\(GfwLocArgs\) \+ sizeof\(uint32_t\*\) == (\d+),", f.read())
    assert m, "locate_gfw_impl.hpp: the argument segment's static_assert"
    return int(m.group(1))


def test_asserted_argument_segment():
    """16 bytes of pointers, two 64-bit strides, six words and 240 ratios,
    then the pointer to the words."""
    assert asserted_argument_bytes() == 16 + 16 + 6 * 4 + 240 * 4 + 8 == 1024


@pytest.mark.skipif(not os.path.exists(OBJ), reason="product objects not built")
@pytest.mark.skipif(not all(CO._tool(t) for t in CO.TOOLS), reason="ROCm LLVM tools absent")
def test_gfw_locate_instances(tmp_path):
    notes = CO.kernel_notes(OBJ, str(tmp_path))
    found = {name: md for name, md in notes if "gfw_locate" in name and name.startswith("_Z")}
    assert sorted(found) == sorted(NAME % w for w in (8, 16, 32)), sorted(found)
    explicit = asserted_argument_bytes()
    for name, md in found.items():
        assert int(md["vgpr_spill_count"]) == 0, (name, md)
        assert int(md.get("sgpr_spill_count", "0")) == 0, (name, md)
        assert int(md.get("private_segment_fixed_size", "0")) == 0, (name, md)
        assert int(md["max_flat_workgroup_size"]) == 64, (name, md)
        # s_0 of the dirty path: 16 registers x 64 lanes
        assert int(md.get("group_segment_fixed_size", "0")) == 4096, (name, md)
        # 8 waves per SIMD: at most 64 VGPRs (and no AGPRs)
        assert int(md["vgpr_count"]) <= 64, (name, md)
        assert int(md.get("agpr_count", "0")) == 0, (name, md)
        # the explicit arguments, and at most the hidden ones behind them
        assert explicit <= int(md["kernarg_segment_size"]) <= explicit + 256, (name, md)
    # bit_locate is still the one instance test_locate_ws_code_object.py expects
    assert len([n for n, _ in notes if "bit_locate" in n and n.startswith("_Z")]) == 1
