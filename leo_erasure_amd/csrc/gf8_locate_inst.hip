// gf8_locate_inst.hip — gf8_locate instances for one input count K (compiled
// once per K = 1..16 with -DLEOEC_GF8_K=K; see locate_impl.hpp).
#include "locate_impl.hpp"

#ifndef LEOEC_GF8_K
#error "compile with -DLEOEC_GF8_K=<1..16>"
#endif

namespace leoec {
namespace detail {

template <>
LocateFn gf8_locate_launcher<LEOEC_GF8_K>(int r) {
  constexpr int K = LEOEC_GF8_K;
  static const LocateFn tbl[kMaxR - 1] = {&launch_gf8_locate_t<K, 2>, &launch_gf8_locate_t<K, 3>,
                                          &launch_gf8_locate_t<K, 4>};
  return tbl[r - 2];
}

}  // namespace detail
}  // namespace leoec
