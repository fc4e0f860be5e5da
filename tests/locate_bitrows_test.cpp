// C entry to locate_build_bitrows (leo_erasure_amd/csrc/locate_bitrows.cpp)
// for tests/test_locate_ws_cpu.py: the builder on bitmatrices no coding class
// produces (a singular block, a singular 2w x 2w minor), which the C ABI
// cannot be given.  Built with locate_bitrows.cpp and codes.cpp, no HIP.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../leo_erasure_amd/csrc/locate_bitrows.hpp"

// bits: (m w) x (k w), one byte per bit, row-major.
extern "C" int locate_bitrows_of(const uint8_t* bits, int k, int m, int w, uint32_t* out) {
  leoec::BitMatrix B;
  B.resize(m * w, k * w);
  for (int r = 0; r < m * w; ++r)
    for (int c = 0; c < k * w; ++c) B.set(r, c, bits[(size_t)r * k * w + c] & 1);
  std::vector<uint32_t> t;
  const int rc = leoec::locate_build_bitrows(B, k, m, w, &t);
  if (rc == 0)
    for (size_t i = 0; i < t.size(); ++i) out[i] = t[i];
  return rc;
}
