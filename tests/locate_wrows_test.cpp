// C entry to locate_build_wrows (leo_erasure_amd/csrc/locate_wrows.cpp) for
// tests/test_locate_gfw_cpu.py: the builder on matrices no coding class
// produces (a zero entry, a singular 2 x 2 minor), which the C ABI cannot be
// given.  Built with locate_wrows.cpp and codes.cpp, no HIP.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../leo_erasure_amd/csrc/locate_wrows.hpp"

extern "C" int locate_wrows_of(const uint32_t* C, int k, int m, int w, uint32_t* out) {
  std::vector<uint32_t> t;
  const int rc = leoec::locate_build_wrows(C, k, m, w, &t);
  if (rc == 0)
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
  return rc;
}
