// scrub_impl.hpp — gf8_heal_list, the rebuild step of leoec_scrub_dev and of
// leoec_heal_ws_dev's fused family, its launch template, and the workspace the
// list lives in.  Included by scrub.hip and heal_ws.hip (dispatch) and
// gf8_scrub_inst.hip (instances, one translation unit per input count K, as
// gf8_heal_inst.hip).
//
// gf8_heal_list is gf8_heal's tile body (gf8_heal_tile, heal_impl.hpp: the one
// function both kernels call) over a list of objects that an earlier launch on
// the stream wrote (scrub_finish, scrub.hip; heal_ws_list, heal_ws_impl.hpp):
// the host does not know how many there are, so the grid is fixed and every
// workgroup walks the items blockIdx.x, blockIdx.x + gridDim.x, ... below
// count x tiles, item -> (object list[item / tiles], tile item % tiles).  With
// a count of 0 every workgroup reads one word and leaves.
// What the loop adds:
//   * the record's tables are staged into LDS once per item, so a barrier
//     stands between an item's last LDS read and the next item's staging;
//   * the loop bound, the list entry and the mask come through readfirstlane
//     and every exit and skip is taken before the item's barriers, so the
//     whole workgroup takes it;
//   * `full` is the item's own: the minimum valid length of the blocks this
//     object reads and writes.
#pragma once

#include <utility>

#include "heal_impl.hpp"

namespace leoec {
namespace detail {

// a: HealArgs of the chunk (lost: the chunk's final words; unhealed, tmap and
// tperm unused); list: indices into the chunk, *count of them, both written by
// an earlier launch on the stream.  count x tiles <= nobj x tiles < 2^31.
template <int K, int R, int WAVES>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WAVES, 8)))
gf8_heal_list(const HealArgs a, const uint32_t* __restrict__ list,
              const uint32_t* __restrict__ count) {
  __shared__ Gf8Lds<K, R> lds;
  const uint32_t items = __builtin_amdgcn_readfirstlane(*count) * a.tiles;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = item / a.tiles;
    const uint32_t tile = item - e * a.tiles;
    const uint32_t obj = __builtin_amdgcn_readfirstlane(list[e]);
    // a listed object has one bit below k + m; any other word is skipped as
    // gf8_heal leaves it, the whole workgroup at once and before any barrier
    const uint32_t mask = __builtin_amdgcn_readfirstlane(a.lost[obj]);
    const bool bad = (uint32_t)__builtin_popcount(mask) > a.m || ((uint64_t)mask >> (a.k + a.m)) != 0ull;
    if (mask == 0u || bad) continue;
    gf8_heal_tile<K, R>(a, lds, blockDim.x * 16u, obj, tile, mask);
    __syncthreads();  // every wave has read this item's tables: the next item may stage its own
  }
}

// Workgroups of gf8_heal_list that a compute unit holds at once under its
// register budget: 4 SIMDs of kGf8HealWaves waves, wg / 64 waves a workgroup
// (its LDS, 2 KiB at most, never binds).
inline uint32_t gf8_heal_list_resident(uint32_t wg) { return 4u * (uint32_t)kGf8HealWaves * 64u / wg; }

// The fixed grid (list_grid) over the objects a describes (a.nobj is the
// caller's): objects x tiles items at most.
template <int K>
int launch_gf8_heal_list_t(HealArgs a, const uint32_t* list, const uint32_t* count, uint32_t cap,
                           hipStream_t s) {
  const Gf8Grid g = gf8_grid_env(a.bs);
  const uint32_t wg = g.wg;
  gf8_set_grid(a, g, a.nobj);
  const uint32_t grid = list_grid((uint64_t)a.nobj * a.tiles, gf8_heal_list_resident(wg), cap);
  return launch_kernel((gf8_heal_list<K, kMaxR, kGf8HealWaves>), dim3(grid), dim3(wg), 0, s, a, list,
                       count);
}

using HealListFn = int (*)(HealArgs, const uint32_t*, const uint32_t*, uint32_t, hipStream_t);

// Defined (explicitly specialised) in gf8_scrub_inst.hip, one TU per K.
template <int K>
HealListFn gf8_heal_list_launcher();

// gf8_heal_list_pick(std::make_index_sequence<kMaxK>{}, k): the launcher of K = k.
template <std::size_t... I>
HealListFn gf8_heal_list_pick(std::index_sequence<I...>, int k) {
  static HealListFn (*const sel[])() = {&gf8_heal_list_launcher<(int)I + 1>...};
  return sel[k - 1]();
}

// The workspace of a call that lists: a header, then one index word per object.
constexpr uint64_t kScrubHeader = 16;  // bytes; word 0: the chunk's count

// Bytes of that workspace for nobj objects; false when that overflows.
inline bool scrub_workspace(uint64_t nobj, uint64_t* bytes) {
  uint64_t words;
  if (__builtin_mul_overflow(nobj, (uint64_t)sizeof(uint32_t), &words) ||
      __builtin_add_overflow(words, (uint64_t)15, &words))
    return false;
  return !__builtin_add_overflow(words & ~(uint64_t)15, kScrubHeader, bytes);
}

// [p, p + n) meets [q, q + qn) (no sum that could wrap).
inline bool overlaps(const void* p, uint64_t n, const void* q, uint64_t qn) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a >= b ? a - b < qn : b - a < n;
}

}  // namespace detail
}  // namespace leoec
