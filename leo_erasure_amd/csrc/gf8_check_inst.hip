// gf8_check_inst.hip — gf8_check instances for one input count K (compiled
// once per K = 1..16 with -DLEOEC_GF8_K=K; see verify_impl.hpp).
#include "verify_impl.hpp"

#ifndef LEOEC_GF8_K
#error "compile with -DLEOEC_GF8_K=<1..16>"
#endif

namespace leoec {
namespace detail {

template <>
CheckFn gf8_check_launcher<LEOEC_GF8_K>(int r) {
  constexpr int K = LEOEC_GF8_K;
  static const CheckFn tbl[kMaxR] = {&launch_gf8_check_t<K, 1>, &launch_gf8_check_t<K, 2>,
                                     &launch_gf8_check_t<K, 3>, &launch_gf8_check_t<K, 4>};
  return tbl[r - 1];
}

}  // namespace detail
}  // namespace leoec
