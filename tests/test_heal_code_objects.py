"""The product library's gf8_heal instances do not spill (CPU test, on the
objects build() leaves in leo_erasure_amd/csrc/_build; modelled on
test_code_objects.py::test_product_kernels_scratch, whose reader of the
kernels' metadata it uses).

gf8_heal keeps gf8_apply's K input columns and R = 4 output columns in VGPRs
and, unlike it, the addresses and valid lengths of its k + 4 blocks in SGPRs
picked per object.  A form whose arithmetic the compiler sinks into the
per-row conditional stores spills 224 VGPRs at K = 10 (heal_impl.hpp); the
shipped one, under a 4-wave register budget, must spill nothing and use no
scratch at any K."""
import glob
import os

import pytest

import test_code_objects as C

FRAG = "_ZN5leoec6detail8gf8_healILi%dELi4ELi4EEE"  # gf8_heal<K, 4, 4 waves>


@pytest.mark.skipif(not glob.glob(os.path.join(C.BUILD, "gf8_heal_k*.o")),
                    reason="product objects not built")
@pytest.mark.skipif(not (C._tool("clang-offload-bundler") and C._tool("llvm-readelf") and
                         C._tool("llvm-objcopy")), reason="ROCm LLVM tools absent")
def test_heal_kernels_do_not_spill(tmp_path):
    found = {}
    for K in range(1, 17):
        obj = os.path.join(C.BUILD, "gf8_heal_k%d.o" % K)
        assert os.path.exists(obj), obj
        for name, md in C.kernel_notes(obj, str(tmp_path)):
            if name.startswith(FRAG % K):
                found[K] = (int(md["vgpr_spill_count"]), int(md.get("private_segment_fixed_size", "0")),
                            int(md["vgpr_count"]))
    assert sorted(found) == list(range(1, 17)), sorted(found)
    assert all(v[:2] == (0, 0) for v in found.values()), found
    # the 4-wave budget: at most 128 VGPRs
    assert max(v[2] for v in found.values()) <= 128, found
