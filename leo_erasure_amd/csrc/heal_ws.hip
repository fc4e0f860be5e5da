// heal_ws.hip — leoec_heal_ws_dev: leoec_heal_dev's bytes for every class,
// with the caller's masks (up to m lost blocks per object), without a host
// round trip and at a cost that follows the number of damaged objects; and
// leoec_heal_bitrows / leoec_heal_wrows, the map of the packet / word classes
// for one lost block of a mask, read from the table the device gets.
//
// Per chunk of objects, on the stream, nothing allocated, uploaded or waited
// for:
//   heal_ws_begin   (heal_ws_impl.hpp) the workspace's header word 0, the
//                   chunk's count, to zero, and ahead of the first chunk both
//                   totals: a launch, not a memset (see there);
//   heal_ws_list    (heal_ws_impl.hpp) unhealed for every object, the indices
//                   of the objects to rebuild appended to the list in the
//                   workspace, both totals added to;
//   the rebuild     from a fixed grid over that list:
//                   gf8_heal_list   (scrub_impl.hpp) leoec_heal_dev's fused
//                                   family, from that call's pattern table and
//                                   cache (heal.hip), unchanged;
//                   gfw_heal_masks  the other vandrs / isars codes,
//                   bit_heal_masks  cauchyrs and liberation: one lost block
//                                   per item from the code's pattern table
//                                   (heal_ws_table.hpp), whose host image is
//                                   built once per code and whose device copy
//                                   is cached per (code, device) in a cache of
//                                   this unit's own (dev_table.hpp).
// A chunk exists only to keep a launch's item count below 2^31.
// Workspace: leoec_scrub_dev's (scrub_impl.hpp), a 16-byte header, then one
// index word per object.  A code is served when its table exists
// (heal_ws_shape: at most 8 MiB), which is decided without a device.
// When the table cache is full the call is heal_ws_list counting only (the
// totals and unhealed, no list), then op_heal_dev's own path, which
// synchronises once.
// This unit is kept out of engine.cpp / capi.cpp for verify.hip's reason: the
// host sanitizer harness links those against stand-in kernels.  The gf_init
// warm-up does not load this unit's kernels either.
#include <map>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "dev_table.hpp"
#include "engine.hpp"
#include "heal_ws_impl.hpp"
#include "knobs.hpp"
#include "scrub_bit_table.hpp"
#include "scrub_impl.hpp"
#include "scrub_steps.hpp"

namespace leoec {

using namespace detail;

namespace {

// leoec_heal_dev's fused family, the other word codes, the packet classes.
enum class HealWsKind { gf8, gfw, bit };

struct HealWsClass {
  HealWsKind kind;
  int per;  // gfw, bit: words per (lost block, survivor) of a record
};

// The class of a configuration whose parameters are valid, and whether this
// call serves it: needs no device.
int heal_ws_served(int coding, int k, int m, int w, HealWsClass* out) {
  if (k + m > kHealWsMaxIds) return LEOEC_E_UNSUPPORTED;
  if (gf8_fused_config(coding, k, m, w)) {  // leoec_heal_dev's table: 8 MB at most
    *out = HealWsClass{HealWsKind::gf8, 0};
    return LEOEC_OK;
  }
  *out = bit_class(coding) ? HealWsClass{HealWsKind::bit, w} : HealWsClass{HealWsKind::gfw, 1};
  return heal_ws_shape(k, m, out->per, nullptr);
}

// The maps of `nwant` lost ids in a record's order (heal_ws_table.hpp).
int heal_ws_rows(const Code& c, int per, const int* surv, const int* want, int nwant,
                 uint32_t* out) {
  const int k = c.k;
  if (per == 1) {
    std::vector<uint32_t> rows;
    const int rc = gf_rows(c, surv, want, nwant, &rows);
    if (rc) return rc;
    if (rows.size() != (size_t)nwant * k) return LEOEC_E_ARG;
    for (size_t i = 0; i < rows.size(); ++i) out[i] = rows[i];
    return LEOEC_OK;
  }
  const int w = c.w, n = k * w;
  std::vector<uint8_t> bits;  // (nwant w) x (k w)
  const int rc = bit_rows(c, surv, want, nwant, &bits);
  if (rc) return rc;
  if (per != w || bits.size() != (size_t)nwant * w * n) return LEOEC_E_ARG;
  // transposed: one word per input packet naming the output packets it feeds
  for (int r = 0; r < nwant; ++r)
    for (int col = 0; col < n; ++col) {
      uint32_t word = 0;
      for (int t = 0; t < w; ++t) word |= (uint32_t)(bits[(size_t)(r * w + t) * n + col] & 1u) << t;
      out[(size_t)r * n + col] = word;
    }
  return LEOEC_OK;
}

// The host image of a code's pattern table, built once and kept with the
// cached Code (get_code never frees one); needs no device.  The device gets a
// copy of it (heal_ws_table), leoec_heal_bitrows and leoec_heal_wrows read its
// records.
int heal_ws_image(const Code* c, int per, const std::vector<uint32_t>** out) {
  struct Entry {
    int rc;
    std::vector<uint32_t> image;
  };
  static std::mutex mu;
  static std::map<const Code*, Entry> cache;
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(c);
  if (it == cache.end()) {
    Entry e;
    const auto rows = [c, per](const int* surv, const int* want, int nwant, uint32_t* r) {
      return heal_ws_rows(*c, per, surv, want, nwant, r);
    };
    e.rc = heal_ws_build_table(c->k, c->m, per, rows, &e.image);
    it = cache.emplace(c, std::move(e)).first;
  }
  *out = &it->second.image;
  return it->second.rc;
}

// The pattern table of the code on the current device (dev_table.hpp), one per
// (coding, k, m, w, device), in a cache of its own: nullptr when it is full,
// and the caller takes op_heal_dev's path.
int heal_ws_table(const Code& c, int per, const uint32_t** out) {
  // at most 16 x 8 MiB of device memory; leaked: never destroyed at exit
  static auto* const cache = new DevTableCache<std::tuple<int, int, int, int>, 16>;
  const auto build = [&](std::vector<uint32_t>* host) {
    const std::vector<uint32_t>* image;
    const int rc = heal_ws_image(&c, per, &image);
    if (!rc) *host = *image;
    return rc;
  };
  return cache->get(std::make_tuple(c.coding, c.k, c.m, c.w), build, out);
}

int op_heal_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                             uint64_t* bytes) {
  int rc = op_layout(coding, k, m, w, size, nullptr, nullptr);
  if (rc) return rc;
  HealWsClass cl;
  if ((rc = heal_ws_served(coding, k, m, w, &cl))) return rc;
  if (!bytes) return LEOEC_E_ARG;
  return scrub_workspace(nobj, bytes) ? LEOEC_OK : LEOEC_E_BAD_SIZE;
}

int op_heal_ws_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                   uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                   const uint32_t* lost, uint32_t* unhealed, uint32_t* totals, void* workspace,
                   uint64_t workspace_bytes, hipStream_t s) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  HealWsClass cl;
  if ((rc = heal_ws_served(coding, k, m, w, &cl))) return rc;
  if (nobj == 0 || bs == 0) return LEOEC_OK;  // leoec_heal_dev's empty batch
  if (!lost || !unhealed || lost == unhealed) return LEOEC_E_ARG;
  if (((uintptr_t)lost & 3u) || ((uintptr_t)unhealed & 3u)) return LEOEC_E_ARG;
  if (!totals || ((uintptr_t)totals & 3u)) return LEOEC_E_ARG;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  if (!workspace || ((uintptr_t)workspace & 15u)) return LEOEC_E_ARG;
  uint64_t need;
  if (!scrub_workspace(nobj, &need)) return LEOEC_E_BAD_SIZE;
  if (workspace_bytes < need) return LEOEC_E_ARG;
  if (overlaps(unhealed, nobj * sizeof(uint32_t), workspace, workspace_bytes) ||
      overlaps(lost, nobj * sizeof(uint32_t), workspace, workspace_bytes) ||
      overlaps(totals, 2 * sizeof(uint32_t), workspace, workspace_bytes))
    return LEOEC_E_ARG;
  if ((rc = device_init())) return rc;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  const uint32_t* table = nullptr;
  if ((rc = cl.kind == HealWsKind::gf8 ? heal_table(*c, &table) : heal_ws_table(*c, cl.per, &table)))
    return rc;
  uint32_t* const header = static_cast<uint32_t*>(workspace);
  uint32_t* const list = header + kScrubHeader / sizeof(uint32_t);
  // tiles of a block (gfw), of a packet (bit); gf8: gf8_max_objects' bound
  const uint32_t ps = cl.kind == HealWsKind::bit ? (uint32_t)(bs / (uint64_t)w) : 0u;
  const uint64_t tiles = cl.kind == HealWsKind::gfw   ? (bs + kGfwHealTile - 1) / kGfwHealTile
                         : cl.kind == HealWsKind::bit ? (ps + kBitHealTile - 1u) / kBitHealTile
                                                      : 0;
  // objects of a launch: items = objects x m x tiles < 2^31 (bs < 2^32, m <= 31)
  uint64_t max_obj = cl.kind == HealWsKind::gf8 ? gf8_max_objects(bs)
                                                : (uint64_t)0x7FFFFFFF / ((uint64_t)m * tiles);
  if (kMeasureBuild && knobs().heal_ws_chunk > 0 && (uint64_t)knobs().heal_ws_chunk < max_obj)
    max_obj = (uint64_t)knobs().heal_ws_chunk;
  if (max_obj == 0) return LEOEC_E_BAD_SIZE;
  const HealListFn gf8 = cl.kind == HealWsKind::gf8 && table
                             ? gf8_heal_list_pick(std::make_index_sequence<kMaxK>{}, k)
                             : nullptr;
  const uint32_t cap = kMeasureBuild && knobs().scrub_grid > 0 ? (uint32_t)knobs().scrub_grid : 0u;
  for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
    const uint64_t no = nobj - o0 < max_obj ? nobj - o0 : max_obj;
    // the totals ahead of the first chunk, the list's count ahead of every one
    if (launch_kernel(heal_ws_begin, dim3(1), dim3(64), 0, s, o0 == 0 ? totals : nullptr,
                      table ? header : nullptr) != LEOEC_OK)
      return LEOEC_E_HIP;
    // no <= 2^31 - 1 words: one grid
    if (launch_kernel(heal_ws_list, dim3((uint32_t)((no + kThreads - 1) / kThreads)), dim3(kThreads),
                      0, s, lost + o0, unhealed + o0, (uint32_t)no, (uint32_t)(k + m), (uint32_t)m,
                      table ? list : nullptr, header, totals) != LEOEC_OK)
      return LEOEC_E_HIP;
    if (!table) continue;
    HealArgs h;
    h.objs = objs + o0 * obj_stride;
    h.obj_stride = obj_stride;
    h.parity = parity + o0 * parity_stride;
    h.parity_stride = parity_stride;
    h.lost = lost + o0;
    h.unhealed = nullptr;
    h.table = table;
    h.size = size;
    h.bs = (uint32_t)bs;  // < 2^32 (check_dev_batch); gfw, bit: a multiple of 16 w
    h.k = (uint32_t)k;
    h.m = (uint32_t)m;
    h.nobj = (uint32_t)no;
    h.tiles = (uint32_t)tiles;  // gf8: the launcher's
    h.tmap = h.tperm = 0;
    if (cl.kind == HealWsKind::gf8) {
      rc = gf8(h, list, header, cap, s);
    } else if (cl.kind == HealWsKind::gfw) {
      GfwHealArgs g;
      g.h = h;
      g.rec_words = heal_ws_record_words(k, m, 1);
      g.red = field(8).mul(0x80u, 2u);  // alpha^8 reduced: the polynomial's low byte
      rc = launch_gfw_heal_masks(w, g, list, header, cap, s);
    } else {
      BitHealArgs a;
      a.h = h;
      a.w = (uint32_t)w;
      a.ps = ps;
      a.rec_words = heal_ws_record_words(k, m, w);
      a.pad = 0;
      rc = launch_bit_heal_masks(a, list, header, cap, s);
    }
    if (rc) return rc;
  }
  if (table) return LEOEC_OK;
  // the table cache is full: unhealed and the totals are final; the rest is
  // leoec_heal_dev's own path (one synchronisation), which writes the same
  // words into unhealed once more
  return op_heal_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, lost,
                     unhealed, s);
}

int op_heal_bitrows(int coding, int k, int m, int w, uint32_t lost_mask, int r, int* surv,
                    uint32_t* rows, int cap) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (!bit_class(coding)) return LEOEC_E_UNSUPPORTED;
  HealWsClass cl;
  if ((rc = heal_ws_served(coding, k, m, w, &cl))) return rc;
  if (((uint64_t)lost_mask >> (k + m)) != 0) return LEOEC_E_BAD_ID;
  const int bits = __builtin_popcount(lost_mask);
  if (bits > m) return LEOEC_E_NOT_ENOUGH_BLOCKS;
  if (r < 0 || r >= bits) return LEOEC_E_ARG;
  const int rw = scrub_bit_row_words(k, w);
  if (!surv || !rows || cap < w * rw) return LEOEC_E_ARG;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  const std::vector<uint32_t>* image;
  if ((rc = heal_ws_image(c, cl.per, &image))) return rc;
  int want[kHealWsMaxIds], nwant = 0;
  const uint32_t* body;
  if ((rc = heal_ws_record(*image, k, m, cl.per, lost_mask, surv, want, &nwant, &body))) return rc;
  // the record's feed words of slot r, transposed back into leoec_scrub_bitrows' rows
  const uint32_t* feed = body + (size_t)r * k * w;
  for (int i = 0; i < w * rw; ++i) rows[i] = 0u;
  for (int col = 0; col < k * w; ++col)
    for (int t = 0; t < w; ++t)
      if ((feed[col] >> t) & 1u) rows[(size_t)t * rw + col / 32] |= 1u << (col % 32);
  return LEOEC_OK;
}

int op_heal_wrows(int coding, int k, int m, int w, uint32_t lost_mask, int r, int* surv,
                  uint32_t* coef, int cap) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (bit_class(coding) || gf8_fused_config(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  HealWsClass cl;
  if ((rc = heal_ws_served(coding, k, m, w, &cl))) return rc;
  if (((uint64_t)lost_mask >> (k + m)) != 0) return LEOEC_E_BAD_ID;
  const int bits = __builtin_popcount(lost_mask);
  if (bits > m) return LEOEC_E_NOT_ENOUGH_BLOCKS;
  if (r < 0 || r >= bits) return LEOEC_E_ARG;
  if (!surv || !coef || cap < k) return LEOEC_E_ARG;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  const std::vector<uint32_t>* image;
  if ((rc = heal_ws_image(c, cl.per, &image))) return rc;
  int want[kHealWsMaxIds], nwant = 0;
  const uint32_t* body;
  if ((rc = heal_ws_record(*image, k, m, cl.per, lost_mask, surv, want, &nwant, &body))) return rc;
  for (int i = 0; i < k; ++i) coef[i] = body[(size_t)r * k + i];
  return LEOEC_OK;
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_heal_wrows(int coding, int k, int m, int w, uint32_t lost_mask, int r, int* surv,
                     uint32_t* coef, int cap) {
  return leoec::guarded(
      [&] { return leoec::op_heal_wrows(coding, k, m, w, lost_mask, r, surv, coef, cap); });
}

int leoec_heal_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_heal_ws_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_heal_ws_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                      uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                      const uint32_t* lost, uint32_t* unhealed, uint32_t* totals, void* workspace,
                      uint64_t workspace_bytes, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_heal_ws_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                 parity_stride, lost, unhealed, totals, workspace, workspace_bytes,
                                 (hipStream_t)stream);
  });
}

int leoec_heal_bitrows(int coding, int k, int m, int w, uint32_t lost_mask, int r, int* surv,
                       uint32_t* rows, int cap) {
  return leoec::guarded(
      [&] { return leoec::op_heal_bitrows(coding, k, m, w, lost_mask, r, surv, rows, cap); });
}

}  // extern "C"
