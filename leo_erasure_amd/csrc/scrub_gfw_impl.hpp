// scrub_gfw_impl.hpp — gfw_heal_list<W>, the rebuild step of
// leoec_scrub_gfw_dev for the GF(2^w) word classes (vandrs w = 16 / 32, vandrs
// / isars w = 8 outside leoec_scrub_dev's k <= 16, m <= 4), and its launch.
// Included by scrub.hip alone.
//
// The kernel rebuilds one named block of every object of a list that an
// earlier launch on the stream wrote (scrub_finish, scrub.hip): the host does
// not know how many there are, so the grid is fixed and every workgroup walks
// the items blockIdx.x, blockIdx.x + gridDim.x, ... below count x tiles,
// item -> (object list[item / tiles], tile item % tiles), as bit_heal_list
// (scrub_bit_impl.hpp).  With a count of 0 every workgroup reads one word and
// leaves.  The item's tile is gfw_heal_tile (gfw_heal_tile.hpp: the one body
// this kernel and gfw_heal_masks share), from the block's record of the code's
// block table (scrub_gfw_table.hpp).
//
// Every exit and skip is taken by the whole wave: the loop bound, the list
// entry and the object's word are read at wave-uniform addresses through the
// constant address space (uniform_word, heal_impl.hpp).
#pragma once

#include "gfw_heal_tile.hpp"
#include "scrub_gfw_table.hpp"

namespace leoec {
namespace detail {

// a: GfwHealArgs with lost = the chunk's final words, table = the code's block
// table and rec_words = scrub_gfw_record_words(k).  list: indices into the
// chunk, *count of them, both written by an earlier launch on the stream.
// count x tiles <= nobj x tiles < 2^31.
template <int W>
__global__ void __launch_bounds__(kGfwHealLanes) __attribute__((amdgpu_waves_per_eu(kGfwHealWaves)))
gfw_heal_list(const GfwHealArgs a, const uint32_t* __restrict__ list,
              const uint32_t* __restrict__ count) {
  const uint32_t tiles = a.h.tiles;
  const uint32_t items = uniform_word(count) * tiles;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint32_t e = item / tiles;
    const uint32_t tile = item - e * tiles;
    const uint32_t obj = uniform_word(list + e);
    // a listed object has exactly one bit below k + m (<= 31); any other word
    // is skipped, the whole wave at once
    const uint32_t word = uniform_word(a.h.lost + obj);
    if (word == 0u || (word & (word - 1u)) != 0u || (word >> (a.h.k + a.h.m)) != 0u) continue;
    const uint32_t block = (uint32_t)__builtin_ctz(word);
    const uint32_t* const rec = a.h.table + (uint64_t)block * a.rec_words;
    gfw_heal_tile<W>(a.h, rec, rec + kScrubGfwIdWords, a.red, obj, block, tile);
  }
}

// The fixed grid (list_grid) over the objects a describes (a.h.nobj and
// a.h.tiles are the caller's): objects x tiles items at most.
inline int launch_gfw_heal_list(int w, const GfwHealArgs& a, const uint32_t* list,
                                const uint32_t* count, uint32_t cap, hipStream_t s) {
  const dim3 g(list_grid((uint64_t)a.h.nobj * a.h.tiles, gfw_heal_list_resident(), cap));
  const dim3 b(kGfwHealLanes);
  if (w == 8) return launch_kernel(gfw_heal_list<8>, g, b, 0, s, a, list, count);
  if (w == 16) return launch_kernel(gfw_heal_list<16>, g, b, 0, s, a, list, count);
  return launch_kernel(gfw_heal_list<32>, g, b, 0, s, a, list, count);
}

}  // namespace detail
}  // namespace leoec
