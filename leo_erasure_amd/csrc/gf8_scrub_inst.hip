// gf8_scrub_inst.hip — the gf8_heal_list instance for one input count K
// (compiled once per K = 1..16 with -DLEOEC_GF8_K=K; see scrub_impl.hpp).
#include "scrub_impl.hpp"

#ifndef LEOEC_GF8_K
#error "compile with -DLEOEC_GF8_K=<1..16>"
#endif

namespace leoec {
namespace detail {

template <>
HealListFn gf8_heal_list_launcher<LEOEC_GF8_K>() {
  return &launch_gf8_heal_list_t<LEOEC_GF8_K>;
}

}  // namespace detail
}  // namespace leoec
