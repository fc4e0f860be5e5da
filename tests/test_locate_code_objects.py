"""The product library's gf8_locate instances do not spill (CPU test, on the
objects build() leaves in leo_erasure_amd/csrc/_build; modelled on
test_heal_code_objects.py, whose reader of the kernels' metadata it shares).

gf8_locate is gf8_check up to the syndromes, under the same 4-wave register
budget, plus a cold branch that multiplies one syndrome by up to 3 K ratios.
That branch must cost the clean path nothing it can be measured by here:
every instance (K = 1..16, R = 2..4) spills no VGPR, uses no scratch and
takes at most 128 VGPRs."""
import glob
import os

import pytest

import test_code_objects as C

FRAG = "_ZN5leoec6detail10gf8_locateILi%dELi%dELi4EEE"  # gf8_locate<K, R, 4 waves>


@pytest.mark.skipif(not glob.glob(os.path.join(C.BUILD, "gf8_locate_k*.o")),
                    reason="product objects not built")
@pytest.mark.skipif(not (C._tool("clang-offload-bundler") and C._tool("llvm-readelf") and
                         C._tool("llvm-objcopy")), reason="ROCm LLVM tools absent")
def test_locate_kernels_do_not_spill(tmp_path):
    found = {}
    for K in range(1, 17):
        obj = os.path.join(C.BUILD, "gf8_locate_k%d.o" % K)
        assert os.path.exists(obj), obj
        for name, md in C.kernel_notes(obj, str(tmp_path)):
            for R in (2, 3, 4):
                if name.startswith(FRAG % (K, R)):
                    found[K, R] = (int(md["vgpr_spill_count"]),
                                   int(md.get("private_segment_fixed_size", "0")),
                                   int(md["vgpr_count"]))
    assert sorted(found) == [(K, R) for K in range(1, 17) for R in (2, 3, 4)], sorted(found)
    assert all(v[:2] == (0, 0) for v in found.values()), found
    # the 4-wave budget: at most 128 VGPRs
    assert max(v[2] for v in found.values()) <= 128, found
