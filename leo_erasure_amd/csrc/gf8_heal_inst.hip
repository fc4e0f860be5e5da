// gf8_heal_inst.hip — the gf8_heal instance for one input count K (compiled
// once per K = 1..16 with -DLEOEC_GF8_K=K; see heal_impl.hpp).
#include "heal_impl.hpp"

#ifndef LEOEC_GF8_K
#error "compile with -DLEOEC_GF8_K=<1..16>"
#endif

namespace leoec {
namespace detail {

template <>
HealFn gf8_heal_launcher<LEOEC_GF8_K>() {
  return &launch_gf8_heal_t<LEOEC_GF8_K>;
}

}  // namespace detail
}  // namespace leoec
