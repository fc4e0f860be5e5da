// heal_ws_impl.hpp — the kernels of leoec_heal_ws_dev (heal_ws.hip, which
// alone includes this): heal_ws_list, the listing step of every class, and the
// rebuild kernels of the classes outside leoec_heal_dev's fused family,
// gfw_heal_masks<W> (vandrs w = 16 / 32, vandrs / isars w = 8 with k > 16 or
// m > 4) and bit_heal_masks (cauchyrs, liberation), with their launches.  The
// fused family rebuilds with gf8_heal_list (scrub_impl.hpp), which takes any
// mask of at most m bits as it is.
//
// heal_ws_list is scrub_finish's compaction (scrub.hip) with heal's predicate:
// the caller's masks are read, unhealed written, and the objects that can be
// rebuilt appended to the list.
//
// gfw_heal_masks and bit_heal_masks are gfw_heal_list's (scrub_gfw_impl.hpp)
// and bit_heal_list's (scrub_bit_impl.hpp) tile bodies, copies as gf8_heal_list
// is one of gf8_heal: those kernels' text, code objects and register tables
// stay as they are.  The lane arithmetic is not copied: gfwheal::mac_in,
// gfwheal::from_domain, gfw_heal_load and gfw_heal_tail are the ones
// gfw_heal_list uses.  What differs:
//   * the record comes from the mask's rank in the code's pattern table
//     (heal_ws_table.hpp), first[p] + sum of C(b_i, i), and holds one map per
//     lost block;
//   * an item is (list entry, lost slot r, tile): one output per item, so the
//     survivors are read once per lost block; an item whose slot lies at or
//     above the mask's bit count is skipped by the whole wave;
//   * the mask's recoverability is tested in 64 bits: at k + m = 32 bit 31 is
//     an ordinary block.
// Every bound, list entry, mask and record word comes through uniform_word
// (heal_impl.hpp).  `full` is the item's own and taken over the object's least
// valid length, that of data block k - 1 (the valid lengths do not grow with
// the id); the lost block is written below its own valid length only; the
// accumulators are zeroed per item.
#pragma once

#include "heal_ws_table.hpp"
#define LEOEC_GFW_HEAL_LIST_NO_LAUNCH  // the lane helpers, not gfw_heal_list's instances
#include "scrub_gfw_impl.hpp"

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
// take their stretch of the list with one atomicAdd per wave on *count
// (list != nullptr) and add their number to totals[0], the others theirs to
// totals[1].  A wave with neither issues no atomic.  No lane leaves early:
// lanes past n hold a clean word, so lane 0 is there to issue the wave's
// atomics.  The order of the list is whatever order the waves arrive in.
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
  const uint64_t b1 = __builtin_amdgcn_ballot_w64(one);
  const uint64_t bm = __builtin_amdgcn_ballot_w64(many);
  if ((b1 | bm) == 0ull) return;  // wave-uniform
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (b1 != 0ull) {
    const uint32_t c = (uint32_t)__builtin_popcountll(b1);
    uint32_t base = 0;
    if (lane == 0u) {
      if (list) base = atomicAdd(count, c);
      atomicAdd(&totals[0], c);
    }
    base = __builtin_amdgcn_readfirstlane(base);
    // the lane's rank among the wave's listed lanes
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b1 >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)b1, 0u));
    if (list && one) list[base + rank] = i;
  }
  if (bm != 0ull && lane == 0u) atomicAdd(&totals[1], (uint32_t)__builtin_popcountll(bm));
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

// ---------------------------------------------------------------------------
// The word classes.

// list: indices into the chunk, *count of them, both written by an earlier
// launch on the stream.  count x m x tiles <= nobj x m x tiles < 2^31.  a:
// GfwHealArgs with table = the code's pattern table and rec_words =
// heal_ws_record_words(k, m, 1).
template <int W>
__global__ void __launch_bounds__(kGfwHealLanes) __attribute__((amdgpu_waves_per_eu(kGfwHealWaves)))
gfw_heal_masks(const GfwHealArgs a, const uint32_t* __restrict__ list,
               const uint32_t* __restrict__ count) {
  const uint32_t listed = uniform_word(count);  // at most the chunk's objects: the list holds no more
  const uint32_t items = (listed < a.h.nobj ? listed : a.h.nobj) * a.h.m * a.h.tiles;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    HealWsItem it;
    if (!heal_ws_item(a.h, list, item, it)) continue;
    const uint32_t block = heal_ws_slot_id(it.mask, it.r);
    const uint32_t* const rec = heal_ws_rec(a.h.table, a.rec_words, it.mask);
    const uint32_t* const coef = rec + kHealWsIdWords + it.r * a.h.k;
    const uint8_t* const ob = a.h.objs + (uint64_t)it.obj * a.h.obj_stride;
    const uint8_t* const pb = a.h.parity + (uint64_t)it.obj * a.h.parity_stride;
    const DevShard out = heal_shard(a.h, ob, pb, block);
    const uint32_t t0 = it.tile * kGfwHealTile;  // < bs
    // nothing of this tile to write: a lost data block with no valid byte, or
    // one that ends before the tile (uniform)
    if (out.valid <= t0) continue;
    const uint32_t off = t0 + threadIdx.x * 16u;
    const uint32_t vlast = heal_shard(a.h, ob, pb, a.h.k - 1u).valid;  // the least of the object's blocks
    const bool full = t0 + kGfwHealTile <= vlast;
    // survivor i of the record; past the last one an empty range (valid 0),
    // the target of the loop's last prefetch: its loads return zeros
    auto shard = [&](uint32_t i) {
      if (i >= a.h.k) return DevShard{ob, 0, 0u, 0u};
      const uint32_t id = (uniform_word(rec + (i >> 2)) >> (8u * (i & 3u))) & 0xFFu;
      return heal_shard(a.h, ob, pb, id);
    };
    auto load = [&](const DevShard& sh, uint32_t (&x)[gfwheal::kRegs]) {
      gfw_heal_load(shard_rsrc(sh.base, 0, sh.valid, 0, 16u), off, x);
    };
    uint32_t acc[1][gfwheal::kRegs];
#pragma unroll
    for (int r = 0; r < gfwheal::kRegs; ++r) acc[0][r] = 0u;
    auto step = [&](uint32_t i, const DevShard& sh, uint32_t (&x)[gfwheal::kRegs]) {
      const uint32_t c = uniform_word(coef + i);
      if (!full) gfw_heal_tail(off, sh.valid, x);
      gfwheal::mac_in<W>(c, x, acc, a.red);
    };
    // two input buffers: survivor i + 1 is loaded into one while survivor i is
    // accumulated in place in the other
    uint32_t bufa[gfwheal::kRegs], bufb[gfwheal::kRegs];
    DevShard cur = shard(0), nx = shard(1);
    load(cur, bufa);
#pragma unroll 1
    for (uint32_t i = 0;; i += 2) {
      load(nx, bufb);  // survivor i + 1 (or empty)
      const DevShard nx2 = shard(i + 2);
      step(i, cur, bufa);
      if (i + 1 >= a.h.k) break;
      load(nx2, bufa);  // survivor i + 2 (or empty)
      const DevShard nx3 = shard(i + 3);
      step(i + 1, nx, bufb);
      if (i + 2 >= a.h.k) break;
      cur = nx2;
      nx = nx3;
    }
    gfwheal::from_domain<W>(acc);
    uint8_t* const base = const_cast<uint8_t*>(out.base);
#pragma unroll
    for (int c = 0; c < kGfwHealLoads; ++c) {
      const uint32_t at = off + (uint32_t)c * (kGfwHealLanes * 16u);
      const u32x4 v = {acc[0][4 * c], acc[0][4 * c + 1], acc[0][4 * c + 2], acc[0][4 * c + 3]};
      if (full) st16<true>(base + at, v);
      else store_guarded(base, at, out.valid, v);
    }
  }
}

// The fixed grid over the objects a describes (a.h.nobj and a.h.tiles are the
// caller's): min(objects x m x tiles, resident workgroups of the device), at
// most `cap` workgroups when cap is not 0 (LEOEC_SCRUB_GRID, measurement
// build).
inline int launch_gfw_heal_masks(int w, const GfwHealArgs& a, const uint32_t* list,
                                 const uint32_t* count, uint32_t cap, hipStream_t s) {
  const uint64_t all = (uint64_t)a.h.nobj * a.h.m * a.h.tiles;
  uint64_t grid = (uint64_t)device_cus() * gfw_heal_list_resident();
  grid = grid < all ? grid : all;
  if (cap != 0u && grid > cap) grid = cap;
  const dim3 g((uint32_t)grid), b(kGfwHealLanes);
  if (w == 8) return launch_kernel(gfw_heal_masks<8>, g, b, 0, s, a, list, count);
  if (w == 16) return launch_kernel(gfw_heal_masks<16>, g, b, 0, s, a, list, count);
  return launch_kernel(gfw_heal_masks<32>, g, b, 0, s, a, list, count);
}

// ---------------------------------------------------------------------------
// The packet classes.  bit_heal_list's geometry (scrub_bit_impl.hpp): one wave
// per workgroup, one 16-byte column of packet offsets per lane, 1 KiB of every
// packet per item, the w output packets in dynamic LDS ([w][64] columns, every
// lane its own slots: no barrier).

constexpr int kBitMasksLanes = 64;
constexpr uint32_t kBitMasksTile = kBitMasksLanes * 16u;  // bytes of every packet per item

// h: HealArgs of the chunk (table: the code's pattern table; tiles: 1 KiB
// tiles of a packet; unhealed, tmap and tperm unused).  ps = bs / w, a
// multiple of 16.
struct BitMasksArgs {
  HealArgs h;
  uint32_t w, ps;
  uint32_t rec_words;  // heal_ws_record_words(k, m, w)
  uint32_t pad;
};

// list, count: as gfw_heal_masks'.
__global__ void __launch_bounds__(kBitMasksLanes)
bit_heal_masks(const BitMasksArgs a, const uint32_t* __restrict__ list,
               const uint32_t* __restrict__ count) {
  extern __shared__ u32x4 bit_masks_acc[];  // [w][kBitMasksLanes]
  u32x4* const acc = bit_masks_acc + threadIdx.x;
  const uint32_t listed = uniform_word(count);  // at most the chunk's objects: the list holds no more
  const uint32_t items = (listed < a.h.nobj ? listed : a.h.nobj) * a.h.m * a.h.tiles;
  for (uint32_t item = blockIdx.x; item < items; item += gridDim.x) {
    HealWsItem it;
    if (!heal_ws_item(a.h, list, item, it)) continue;
    const uint32_t block = heal_ws_slot_id(it.mask, it.r);
    const uint32_t* const rec = heal_ws_rec(a.h.table, a.rec_words, it.mask);
    const uint32_t* const feed = rec + kHealWsIdWords + it.r * a.h.k * a.w;
    const uint8_t* const ob = a.h.objs + (uint64_t)it.obj * a.h.obj_stride;
    const uint8_t* const pb = a.h.parity + (uint64_t)it.obj * a.h.parity_stride;
    const DevShard out = heal_shard(a.h, ob, pb, block);
    const uint32_t t0 = it.tile * kBitMasksTile;  // < ps
    // nothing of this tile to write: a lost data block with no valid byte, or
    // one whose every packet ends before the tile (uniform)
    if (out.valid <= t0) continue;
    const uint32_t off = t0 + threadIdx.x * 16u;
    const bool in = off < a.ps;  // ps is a multiple of 16: the column lies inside the packet
    // lanes past the packet read the tile's first column and store nothing
    const uint32_t col = in ? off : t0;
    const uint32_t vlast = heal_shard(a.h, ob, pb, a.h.k - 1u).valid;  // the least of the object's blocks
    const bool full = t0 + kBitMasksTile <= a.ps &&
                      (uint64_t)(a.w - 1u) * a.ps + t0 + kBitMasksTile <= vlast;
    for (uint32_t r = 0; r < a.w; ++r) acc[r * kBitMasksLanes] = u32x4{0u, 0u, 0u, 0u};
    for (uint32_t i = 0; i < a.h.k; ++i) {
      const uint32_t id = (uniform_word(rec + (i >> 2)) >> (8u * (i & 3u))) & 0xFFu;
      const DevShard sh = heal_shard(a.h, ob, pb, id);
      const auto rs = shard_rsrc(sh.base, 0, sh.valid, 0, 16u);
      const uint32_t* const masks = feed + i * a.w;
      for (uint32_t c = 0; c < a.w; ++c) {
        const uint32_t mask = uniform_word(masks + c);
        if (mask == 0u) continue;  // uniform
        const uint32_t o = c * a.ps + col;  // < bs
        u32x4 v;
        if (full) v = ld16<true>(sh.base + o);
        else v = clip_guarded(__builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 2), o, sh.valid);
        for (uint32_t t = mask; t != 0u; t &= t - 1u) {
          u32x4* const p = acc + (uint32_t)__builtin_ctz(t) * kBitMasksLanes;
          const u32x4 x = *p;
          *p = u32x4{x[0] ^ v[0], x[1] ^ v[1], x[2] ^ v[2], x[3] ^ v[3]};
        }
      }
    }
    uint8_t* const base = const_cast<uint8_t*>(out.base);
    for (uint32_t r = 0; r < a.w; ++r) {
      const u32x4 v = acc[r * kBitMasksLanes];
      const uint32_t o = r * a.ps + col;
      if (full) st16<true>(base + o, v);
      else if (in) store_guarded(base, o, out.valid, v);
    }
  }
}

// Workgroups of bit_heal_masks that a compute unit holds at once: one wave
// each, 32 waves a compute unit, w KiB of its 160 KiB of LDS each.
inline uint32_t bit_heal_masks_resident(uint32_t w) {
  const uint32_t by_lds = 160u / w;  // w <= 32
  return by_lds < 32u ? by_lds : 32u;
}

// The fixed grid, as launch_gfw_heal_masks'.
inline int launch_bit_heal_masks(const BitMasksArgs& a, const uint32_t* list, const uint32_t* count,
                                 uint32_t cap, hipStream_t s) {
  const uint64_t all = (uint64_t)a.h.nobj * a.h.m * a.h.tiles;
  uint64_t grid = (uint64_t)device_cus() * bit_heal_masks_resident(a.w);
  grid = grid < all ? grid : all;
  if (cap != 0u && grid > cap) grid = cap;
  const size_t lds = (size_t)a.w * kBitMasksLanes * sizeof(u32x4);  // <= 32 KiB
  return launch_kernel(bit_heal_masks, dim3((uint32_t)grid), dim3(kBitMasksLanes), lds, s, a, list,
                       count);
}

}  // namespace detail
}  // namespace leoec
