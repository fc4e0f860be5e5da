// tile_maps.hpp — workgroup-id -> tile remaps shared by the streaming kernels
// (kernels_impl.hpp, gfbit_inst.hip, gfs_inst.hip) and the launch geometry of
// the gf8 kernels that picks one (gf8_grid).  Portable C++ (host and device):
// tests/tile_maps_test.cpp checks on the CPU that every map is a bijection on
// [0, n) for the shapes the launchers use, and pins gf8_grid at the
// boundaries of its rules.
//
// The hardware dispatcher deals workgroup ids round-robin over the 8 XCDs of
// an MI355X (cdna_hip_programming.md T1): id b runs on XCD b % 8 as that
// XCD's (b / 8)-th workgroup.  Each XCD has its own L2, so which ids land on
// one XCD decides which tiles share an L2.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define LEOEC_TM_HD __host__ __device__ __forceinline__
#else
#define LEOEC_TM_HD inline
#endif

namespace leoec {
namespace detail {

constexpr uint32_t kXcds = 8;

// XCD-grouping: XCD x gets the contiguous id range [start(x), start(x+1)).
LEOEC_TM_HD uint32_t xcd_group(uint32_t b, uint32_t n) {
  const uint32_t q = n / kXcds, r = n % kXcds, x = b % kXcds;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / kXcds;
}

// Interleave groups of `tiles` consecutive ids over the XCDs: XCD x takes
// groups g = x (mod 8), each group's ids in order.  With `tiles` = tiles per
// object this keeps every object on one XCD while the 8 XCDs work on
// neighbouring objects (xcd_obj_map, tile map 3); with `tiles` = a run length
// it deals runs of consecutive tiles of large blocks over the XCDs (tile map
// 4).  Ids past the last whole round of 8 groups keep their place.
LEOEC_TM_HD uint32_t xcd_obj_map(uint32_t b, uint32_t n, uint32_t tiles) {
  const uint32_t full = (n / tiles / kXcds) * kXcds * tiles;
  if (b >= full) return b;
  const uint32_t x = b % kXcds, i = b / kXcds;
  return ((i / tiles) * kXcds + x) * tiles + i % tiles;
}

// Object-interleaved XCD map: with the dispatcher dealing workgroup ids
// round-robin over the 8 XCDs, give XCD x the objects o = x (mod 8) with all
// of an object's `tiles` tiles in order, so neighbouring tiles (which share
// the partial cache lines of packets that start mid-line) meet in one L2 at
// about the same time, while the 8 XCDs still work on neighbouring objects.
// Ids past the last whole group of 8 objects keep their place.  Used when an
// object has at most kObjMapMaxTiles tiles (1 MiB objects: +2-3 % on gf8,
// +1-2 % on cauchyrs, +4-8 % on liberation); with many tiles per object
// (objects of 4 MiB and up) it measured 2-4 % slower than dispatch order.
constexpr uint32_t kObjMapMaxTiles = 64;
// Blocks of at least kSegMapMinTiles tiles (32 MiB objects: 3,277 tiles of
// 1 KiB; 64 MiB: 6,554) run gf8_apply under tile map 4 with groups of
// kSegMapGroup tiles: XCD x takes every 8th run of 128 consecutive tiles
// (128 KiB of each block), so each L2 streams whole 128 KiB stretches of the
// 14 blocks instead of every 8th KiB.  RS(10,4,8), one process each
// (profiles/r02_v13_ab_tmap4_*.log): 64 x 64 MiB 0.720 / 0.734 -> 0.743 /
// 0.744 of HBM peak (encode / decode), 128 x 32 MiB 0.722 / 0.736 -> 0.743 /
// 0.742; 16 MiB (1,639 tiles) unchanged and 4 MiB (410 tiles) 1 % slower, so
// smaller blocks keep id order.
constexpr uint32_t kSegMapMinTiles = 2048;
constexpr uint32_t kSegMapGroup = 128;
// Blocks larger than this run the gf8 kernels with 64-lane workgroups: 1 MiB
// objects (bs 104,960) keep 256 lanes, 2 MiB (209,792) and up take 64.
constexpr uint64_t kGf8NarrowBytes = 160 * 1024;

// Launch geometry of the one-tile-per-workgroup gf8 kernels (gf8_apply,
// gf8_check, gf8_locate, gf8_heal): lanes per workgroup, tiles per block and
// the tile map (Gf8Args::tmap / tperm).  Host only.
struct Gf8Grid {
  uint32_t wg, tiles, tmap, tperm;
};
//  wg     wg_default lanes, or 64 lanes (1 KiB tiles) for blocks above
//         kGf8NarrowBytes, where they measured 2-8 % faster (block
//         size sweep); force_wg (LEOEC_GF8_WG) = 64 | 256 forces one (A/B,
//         parity tests).  Only forms with one column per lane and no
//         persistent grid can change width (width_free); cpt = columns per lane.
//  tmap   tmap_knob (LEOEC_GF8_TMAP) when set (tmap_set) or non-zero; else the
//         shipped choice: 3 up to kObjMapMaxTiles tiles, 4 with groups of
//         kSegMapGroup from kSegMapMinTiles, 0 between.  tgroup > 0
//         (LEOEC_GF8_TGROUP) overrides the group of map 4.  Map 2 takes a
//         stride ~ tiles / 16 coprime with tiles (a bijection on the tiles).
inline Gf8Grid gf8_grid(uint64_t block_size, int cpt, bool width_free, uint32_t wg_default,
                        int force_wg, int tmap_knob, bool tmap_set, int tgroup) {
  Gf8Grid g;
  g.wg = wg_default;
  if (width_free && (force_wg == 64 || (force_wg == 0 && block_size > kGf8NarrowBytes))) g.wg = 64;
  const uint32_t tb = g.wg * 16u * (uint32_t)cpt;
  g.tiles = (uint32_t)((block_size + tb - 1) / tb);
  g.tmap = (uint32_t)tmap_knob;
  g.tperm = 1;
  if (g.tmap == 0 && !tmap_set) {
    if (g.tiles <= kObjMapMaxTiles) {
      g.tmap = 3;
    } else if (g.tiles >= kSegMapMinTiles) {
      g.tmap = 4;
      g.tperm = kSegMapGroup;
    }
  }
  if (g.tmap == 4 && tgroup > 0) g.tperm = (uint32_t)tgroup;
  if (g.tmap == 2) {
    uint32_t q = g.tiles / 16u + 1u;
    auto gcd = [](uint32_t x, uint32_t y) { while (y) { const uint32_t t = x % y; x = y; y = t; } return x; };
    while (gcd(q, g.tiles) != 1u) ++q;
    g.tperm = q % g.tiles ? q % g.tiles : 1u;
  }
  return g;
}

// Lane geometry of the packet kernels (gfbit_apply, gfb2_apply): block bytes
// bs = w packets of ps = bs / w bytes; a WG-lane workgroup (tile) covers
// WG * LB bytes at the same offset of every packet of one object, lane l the
// LB bytes at packet offset tile * WG * LB + l * LB.  Lanes at or past ps do
// nothing.  tests/tile_maps_test.cpp checks, for every launch shape, that the
// lanes write each valid output byte once and never read or write past a
// block's valid length rounded up to the lane's chunk.
LEOEC_TM_HD uint32_t packet_tiles(uint32_t ps, uint32_t wg, uint32_t lb) {
  return (ps + wg * lb - 1u) / (wg * lb);
}
LEOEC_TM_HD uint32_t packet_lane_off(uint32_t tile, uint32_t lane, uint32_t wg, uint32_t lb) {
  return tile * (wg * lb) + lane * lb;
}
// Data bytes of packet x in a block whose first `valid` bytes are data (the
// rest of the block reads as zero and is never stored).
LEOEC_TM_HD uint32_t packet_valid(uint32_t valid, uint32_t x, uint32_t ps) {
  const uint32_t pk = x * ps;
  return valid > pk ? valid - pk : 0u;
}

}  // namespace detail
}  // namespace leoec
