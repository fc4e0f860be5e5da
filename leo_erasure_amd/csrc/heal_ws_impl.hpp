// heal_ws_impl.hpp — the kernels of leoec_heal_ws_dev (heal_ws.hip, which
// alone includes this): heal_ws_list, the listing step of every class, and the
// rebuild kernels of the classes outside leoec_heal_dev's fused family,
// gfw_heal_masks<W> (vandrs w = 16 / 32, vandrs / isars w = 8 with k > 16 or
// m > 4) and bit_heal_masks (cauchyrs, liberation), with their launches.  The
// fused family rebuilds with gf8_heal_list (scrub_impl.hpp), which takes any
// mask of at most m bits as it is.
//
// heal_ws_list is scrub_finish's compaction (list_append, heal_impl.hpp) with
// heal's predicate: the caller's masks are read, unhealed written, and the
// objects that can be rebuilt appended to the list.
//
// gfw_heal_masks and bit_heal_masks run the tile bodies gfw_heal_list and
// bit_heal_list run: gfw_heal_tile (gfw_heal_tile.hpp) and bit_heal_tile
// (bit_heal_tile.hpp).  What differs is where an item's record comes from:
//   * the record comes from the mask's rank in the code's pattern table
//     (heal_ws_table.hpp), first[p] + sum of C(b_i, i), and holds one map per
//     lost block;
//   * an item is (list entry, lost slot r, tile): one output per item, so the
//     survivors are read once per lost block; an item whose slot lies at or
//     above the mask's bit count is skipped by the whole wave;
//   * the mask's recoverability is tested in 64 bits: at k + m = 32 bit 31 is
//     an ordinary block.
// Every bound, list entry, mask and record word comes through uniform_word
// (heal_impl.hpp).
#pragma once

#include "bit_heal_tile.hpp"
#include "gfw_heal_tile.hpp"
#include "heal_ws_table.hpp"

namespace leoec {
namespace detail {

// The chunk's first launch: the list's count to zero (count != nullptr) and,
// ahead of the first chunk, both totals (totals != nullptr).  A launch and not
// hipMemsetAsync: captured into a graph, this call's memsets replayed with a
// wrong fill byte from the second replay on (The workspace form:
// the totals came out as 0x60606060 + the count); a kernel's arguments are
// copied when the launch is captured and its stores replay as they were.
__global__ void __launch_bounds__(64)
heal_ws_begin(uint32_t* __restrict__ totals, uint32_t* __restrict__ count) {
  if (totals && threadIdx.x < 2u) totals[threadIdx.x] = 0u;
  if (count && threadIdx.x == 2u) *count = 0u;
}

// One lane per object of the chunk.  unhealed[i] = 0 for a clean or
// recoverable mask, the mask for any other; the recoverable, non-zero objects
// are listed and counted into totals[0], the others into totals[1]
// (list_append).
__global__ void __launch_bounds__(kThreads)
heal_ws_list(const uint32_t* __restrict__ lost, uint32_t* __restrict__ unhealed, uint32_t n,
             uint32_t ids, uint32_t m, uint32_t* __restrict__ list, uint32_t* __restrict__ count,
             uint32_t* __restrict__ totals) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  const bool in = i < n;
  const uint32_t v = in ? lost[i] : 0u;
  // ids <= 32: the shift is taken in 64 bits, bit 31 is a block like any other
  const bool many = (uint32_t)__builtin_popcount(v) > m || ((uint64_t)v >> ids) != 0ull;
  const bool one = v != 0u && !many;
  if (in) unhealed[i] = many ? v : 0u;
  list_append(one, many, i, list, count, totals);
}

// What an item of the rebuild kernels is: entry e of the list, lost slot r of
// its mask, tile `tile` of the block.
struct HealWsItem {
  uint32_t obj, mask, r, tile;
};

// item -> (list entry, slot, tile), the entry's object and its mask
// (wave-uniform).  false: nothing to do for this item, which the whole wave
// skips: an index past the chunk or a mask that is clean or cannot be healed
// (never listed), or a slot at or above the mask's bit count.
__device__ __forceinline__ bool heal_ws_item(const HealArgs& h, const uint32_t* list, uint32_t item,
                                             HealWsItem& it) {
  const uint32_t per = h.m * h.tiles;
  const uint32_t e = item / per;
  const uint32_t rem = item - e * per;
  it.r = rem / h.tiles;
  it.tile = rem - it.r * h.tiles;
  it.obj = uniform_word(list + e);
  if (it.obj >= h.nobj) return false;  // never listed: nothing is read or written past the chunk
  it.mask = uniform_word(h.lost + it.obj);
  const uint32_t bits = (uint32_t)__builtin_popcount(it.mask);
  if (it.mask == 0u || bits > h.m || ((uint64_t)it.mask >> (h.k + h.m)) != 0ull) return false;
  return it.r < bits;
}

// The id of lost slot r of the mask (r below its bit count).
__device__ __forceinline__ uint32_t heal_ws_slot_id(uint32_t mask, uint32_t r) {
  for (uint32_t j = 0; j < r; ++j) mask &= mask - 1u;
  return (uint32_t)__builtin_ctz(mask);
}

// The mask's record in the image T (heal_ws_table.hpp), rw words a record:
// first[bits] + sum of C(b_i, i) over the set bits ascending.
__device__ __forceinline__ const uint32_t* heal_ws_rec(const uint32_t* T, uint32_t rw, uint32_t mask) {
  uint32_t idx = uniform_word(T + kHealWsFirst + (uint32_t)__builtin_popcount(mask));
  uint32_t i = 1;
  for (uint32_t rest = mask; rest != 0u; rest &= rest - 1u, ++i)
    idx += uniform_word(T + kHealWsBinom + (uint32_t)__builtin_ctz(rest) * kHealWsBinomCols + i);
  return T + kHealWsHeaderWords + (uint64_t)idx * rw;
}

// Items of a launch over the list: at most the chunk's objects are listed, the
// list holds no more.
__device__ __forceinline__ uint32_t heal_ws_items(const HealArgs& h, const uint32_t* count) {
  const uint32_t listed = uniform_word(count);
  return (listed < h.nobj ? listed : h.nobj) * h.m * h.tiles;
}

// The word classes.  list: indices into the chunk, *count of them, both
// written by an earlier launch on the stream.  count x m x tiles <= nobj x m x
// tiles < 2^31.  a: GfwHealArgs with table = the code's pattern table and
// rec_words = heal_ws_record_words(k, m, 1).
template <int W>
__global__ void __launch_bounds__(kGfwHealLanes) __attribute__((amdgpu_waves_per_eu(kGfwHealWaves)))
gfw_heal_masks(const GfwHealArgs a, const uint32_t* __restrict__ list,
               const uint32_t* __restrict__ count) {
  const uint32_t items = heal_ws_items(a.h, count);
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    HealWsItem it;
    if (!heal_ws_item(a.h, list, item, it)) continue;
    const uint32_t block = heal_ws_slot_id(it.mask, it.r);
    const uint32_t* const rec = heal_ws_rec(a.h.table, a.rec_words, it.mask);
    gfw_heal_tile<W>(a.h, rec, rec + kHealWsIdWords + it.r * a.h.k, a.red, it.obj, block, it.tile);
  }
}

// The fixed grid (list_grid) over the objects a describes (a.h.nobj and
// a.h.tiles are the caller's): objects x m x tiles items at most.
inline int launch_gfw_heal_masks(int w, const GfwHealArgs& a, const uint32_t* list,
                                 const uint32_t* count, uint32_t cap, hipStream_t s) {
  const dim3 g(list_grid((uint64_t)a.h.nobj * a.h.m * a.h.tiles, gfw_heal_list_resident(), cap));
  const dim3 b(kGfwHealLanes);
  if (w == 8) return launch_kernel(gfw_heal_masks<8>, g, b, 0, s, a, list, count);
  if (w == 16) return launch_kernel(gfw_heal_masks<16>, g, b, 0, s, a, list, count);
  return launch_kernel(gfw_heal_masks<32>, g, b, 0, s, a, list, count);
}

// The packet classes.  list, count: as gfw_heal_masks'.  a: BitHealArgs with
// table = the code's pattern table and rec_words = heal_ws_record_words(k, m, w).
__global__ void __launch_bounds__(kBitHealLanes)
bit_heal_masks(const BitHealArgs a, const uint32_t* __restrict__ list,
               const uint32_t* __restrict__ count) {
  extern __shared__ u32x4 bit_masks_acc[];  // [w][kBitHealLanes]
  u32x4* const acc = bit_masks_acc + threadIdx.x;
  const uint32_t items = heal_ws_items(a.h, count);
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    HealWsItem it;
    if (!heal_ws_item(a.h, list, item, it)) continue;
    const uint32_t block = heal_ws_slot_id(it.mask, it.r);
    const uint32_t* const rec = heal_ws_rec(a.h.table, a.rec_words, it.mask);
    bit_heal_tile(a.h, a.w, a.ps, acc, rec, rec + kHealWsIdWords + it.r * a.h.k * a.w, it.obj, block,
                  it.tile);
  }
}

// The fixed grid, as launch_gfw_heal_masks'.
inline int launch_bit_heal_masks(const BitHealArgs& a, const uint32_t* list, const uint32_t* count,
                                 uint32_t cap, hipStream_t s) {
  const uint32_t grid =
      list_grid((uint64_t)a.h.nobj * a.h.m * a.h.tiles, bit_heal_list_resident(a.w), cap);
  return launch_kernel(bit_heal_masks, dim3(grid), dim3(kBitHealLanes), bit_heal_lds(a.w), s, a, list,
                       count);
}

}  // namespace detail
}  // namespace leoec
