"""bit_locate, the kernel behind leoec_locate_ws_dev's bitmatrix path (CPU
test, on the objects build() leaves in leo_erasure_amd/csrc/_build).

The kernel takes w as a runtime value and keeps the w syndrome packets of its
dirty path in LDS, so that no register array is indexed by w: it must spill no
VGPR and use no scratch (a spilling kernel's first launch makes the runtime
back the whole device's scratch, test_code_objects.py).  Its ratio table is a
kernel argument: the whole argument segment stays under 4 KiB.  The metadata
is read as test_code_objects.py reads it, with the ROCm LLVM tools."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "leo_erasure_amd", "csrc", "_build", "locate.o")
LLVM = "/opt/rocm/lib/llvm/bin"
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def kernel_notes(obj, tmp):
    """[(kernel name, {metadata key: value})] of the gfx950 code object in obj."""
    fat = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", obj, os.devnull],
                   check=True, capture_output=True)
    targets = subprocess.run([_tool("clang-offload-bundler"), "--list", "--type=o", f"--input={fat}"],
                             check=True, capture_output=True, text=True).stdout.split()
    tgt = [t for t in targets if "gfx950" in t]
    assert tgt, (obj, targets)
    co = fat + ".co"
    subprocess.run([_tool("clang-offload-bundler"), "--type=o", f"--targets={tgt[0]}",
                    f"--input={fat}", f"--output={co}", "--unbundle"], check=True, capture_output=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True,
                           text=True).stdout
    # one kernel's keys run, sorted, from .agpr_count to .wavefront_size, its
    # .name in the middle (.kernarg_segment_size before it, .vgpr_count
    # after); the first value of a key wins, so an argument's own keys do not
    # replace the kernel's.  Arguments' .name lines give entries too: the
    # caller picks kernels by their mangled names.
    lines = notes.splitlines()
    kernels = []
    for at, line in enumerate(lines):
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if not m:
            continue
        lo = at
        while lo > 0 and not re.match(r"\s+\.wavefront_size:", lines[lo - 1]):
            lo -= 1
        hi = at
        while hi + 1 < len(lines) and not re.match(r"\s+\.wavefront_size:", lines[hi]):
            hi += 1
        md = {}
        for x in lines[lo:hi + 1]:
            kv = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", x)
            if kv and kv.group(1) not in md:
                md[kv.group(1)] = kv.group(2)
        kernels.append((m.group(1), md))
    return kernels


@pytest.mark.skipif(not os.path.exists(OBJ), reason="product objects not built")
@pytest.mark.skipif(not all(_tool(t) for t in TOOLS), reason="ROCm LLVM tools absent")
def test_bit_locate_does_not_spill(tmp_path):
    found = [(name, md) for name, md in kernel_notes(OBJ, str(tmp_path))
             if "bit_locate" in name and name.startswith("_Z")]
    assert len(found) == 1, [name for name, _ in found]  # one instance, not one per w
    name, md = found[0]
    assert int(md["vgpr_spill_count"]) == 0, md
    assert int(md.get("sgpr_spill_count", "0")) == 0, md
    assert int(md.get("private_segment_fixed_size", "0")) == 0, md
    # LDS is sized at the launch (w packets of 64 lanes x 16 B), none static
    assert int(md.get("group_segment_fixed_size", "0")) == 0, md
    assert int(md["max_flat_workgroup_size"]) == 64, md
    # the ratio table (3 KiB) and the rest of the arguments, hidden ones included
    assert 3072 < int(md["kernarg_segment_size"]) < 4096, md
