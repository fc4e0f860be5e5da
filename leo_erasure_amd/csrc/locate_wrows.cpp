// locate_wrows.cpp — see locate_wrows.hpp.  Host only (no HIP includes).
#include "locate_wrows.hpp"

#include "../../include/leoec.h"
#include "codes.hpp"

namespace leoec {

int locate_build_wrows(const uint32_t* C, int k, int m, int w, std::vector<uint32_t>* out) {
  if (k < 1 || m < 2 || (w != 8 && w != 16 && w != 32)) return LEOEC_E_UNSUPPORTED;
  const Field& F = field(w);
  const uint32_t keep = w == 32 ? 0xFFFFFFFFu : (1u << w) - 1u;
  auto at = [&](int i, int j) { return C[(size_t)i * k + j] & keep; };
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < k; ++j)
      if (at(i, j) == 0) return LEOEC_E_UNSUPPORTED;
  for (int i0 = 0; i0 < m; ++i0)
    for (int i1 = i0 + 1; i1 < m; ++i1)
      for (int j0 = 0; j0 < k; ++j0)
        for (int j1 = j0 + 1; j1 < k; ++j1)
          if (F.mul(at(i0, j0), at(i1, j1)) == F.mul(at(i0, j1), at(i1, j0)))
            return LEOEC_E_UNSUPPORTED;
  out->assign((size_t)(m - 1) * k, 0u);
  for (int i = 1; i < m; ++i)
    for (int j = 0; j < k; ++j) (*out)[(size_t)(i - 1) * k + j] = F.div(at(i, j), at(0, j));
  return LEOEC_OK;
}

}  // namespace leoec
