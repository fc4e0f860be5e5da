// C entry to locate_build_rows (leo_erasure_amd/csrc/locate_rows.cpp) for
// tests/test_locate_cpu.py: the builder on matrices no coding class produces
// (a zero entry, a singular 2 x 2 minor), which the C ABI cannot be given.
// Built with locate_rows.cpp and codes.cpp, no HIP.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../leo_erasure_amd/csrc/locate_rows.hpp"

extern "C" int locate_rows_of(const uint32_t* C, int k, int m, uint32_t* out) {
  std::vector<uint32_t> t;
  const int rc = leoec::locate_build_rows(C, k, m, &t);
  if (rc == 0)
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
  return rc;
}
