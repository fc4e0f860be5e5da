// scrub.hip — leoec_scrub_dev: find the inconsistent objects of a device
// batch, name the damaged block of each and rebuild it in place, in one call
// and without a host round trip: leoec_locate_dev's words and leoec_heal_dev's
// bytes, at a cost that follows the number of damaged objects.
//
// Served: what leoec_locate_dev serves.  Per chunk of objects (gf8_max_objects),
// on the stream, nothing allocated, uploaded or waited for:
//   locate          op_locate_dev's memset + gf8_locate (locate.hip), with
//   scrub_finish    below in locate_finish's place: the final word of every
//                   object, the indices of the objects that name one block
//                   appended to a list in the workspace (header word 0: their
//                   count), both totals added to;
//   gf8_heal_list   (scrub_impl.hpp) gf8_heal's tile over that list from a
//                   fixed grid.
// Workspace: a 16-byte header, then one index word per object.
// When heal's table cache is full (heal.hip) the call is the composition
// itself: op_locate_dev with scrub_finish counting only, then op_heal_dev's
// generic path with the index words as its `unhealed`, which synchronises once.
//
// leoec_scrub_ws_dev adds the bitmatrix classes (cauchyrs, liberation, m >= 2,
// k + m <= 31, (m - 1) k w <= 768) and forwards everything else to
// leoec_scrub_dev.  Per chunk of objects that the encode region holds:
//   locate          op_locate_ws_dev's encode, memset and bit_locate;
//   scrub_finish    as above;
//   bit_heal_list   (scrub_bit_impl.hpp) one named block of every listed
//                   object from the code's block table (scrub_bit_table.hpp),
//                   from a fixed grid.
// Workspace: the 16-byte header, one index word per object (rounded up to 16
// bytes), then the encode region, m bs bytes per object of a chunk (ws_pass.hpp).
// The block tables are cached per (code, device) as heal's are (dev_table.hpp),
// in a cache of their own; when it is full the call is the composition:
// op_locate_ws_dev with scrub_finish counting only, then op_heal_dev's generic
// path.
//
// leoec_scrub_gfw_dev adds the GF(2^w) word classes in the same way (vandrs
// w = 16 / 32; vandrs / isars w = 8 with k > 16 or m > 4; m >= 2, k + m <= 31)
// and forwards everything else to leoec_scrub_ws_dev.  Per chunk:
//   locate          op_locate_gfw_dev's encode, memset and gfw_locate;
//   scrub_finish    as above;
//   gfw_heal_list   (scrub_gfw_impl.hpp) one named block of every listed
//                   object from the code's block table (scrub_gfw_table.hpp),
//                   from a fixed grid.
// Workspace and table cache as leoec_scrub_ws_dev's (a cache of its own, under
// 5 KB a table); when it is full the call is op_locate_gfw_dev with
// scrub_finish counting only, then op_heal_dev's generic path.
// All three calls are one function, scrub_run: one ScrubSteps in the locate
// call, which differs between them (ScrubKind) in the encode bytes of its
// workspace check, the table it asks for and the heal-list kernel it launches.
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
#include "knobs.hpp"
#include "scrub_bit_impl.hpp"
#include "scrub_gfw_impl.hpp"
#include "scrub_impl.hpp"
#include "scrub_steps.hpp"
#include "ws_pass.hpp"

namespace leoec {

using namespace detail;

namespace {

// locate_finish (locate.hip) with the compaction in it.  One word per lane, in
// place: all ones -> 0, exactly one bit -> kept, anything else ->
// LEOEC_LOCATE_MANY.  The single-bit words are listed and counted into
// totals[0], the LEOEC_LOCATE_MANY words into totals[1] (list_append,
// heal_impl.hpp): a clean batch writes its words and nothing else.
__global__ void __launch_bounds__(kThreads)
scrub_finish(uint32_t* __restrict__ words, uint32_t n, uint32_t* __restrict__ list,
             uint32_t* __restrict__ count, uint32_t* __restrict__ totals) {
  const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  const bool in = i < n;
  const uint32_t v = in ? words[i] : 0xFFFFFFFFu;
  const uint32_t f = v == 0xFFFFFFFFu ? 0u : (v != 0u && (v & (v - 1u)) == 0u) ? v : LEOEC_LOCATE_MANY;
  if (in) words[i] = f;
  // (no single-bit word is LEOEC_LOCATE_MANY's own bit: k + m <= 20 for
  // leoec_scrub_dev, <= 31 for leoec_scrub_ws_dev and leoec_scrub_gfw_dev,
  // which refuse k + m = 32 for this line's sake)
  const bool many = f == LEOEC_LOCATE_MANY;
  const bool one = f != 0u && !many;
  list_append(one, many, i, list, count, totals);
}

int op_scrub_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                           uint64_t* bytes) {
  // leoec_locate_dev's statuses, none of which needs a device: an empty batch
  // with no buffers goes through its parameter and served tests and ends there
  const int rc = op_locate_dev(coding, k, m, w, nullptr, 0, size, 0, nullptr, 0, nullptr, nullptr,
                               nullptr);
  if (rc) return rc;
  if (!bytes) return LEOEC_E_ARG;
  return scrub_workspace(nobj, bytes) ? LEOEC_OK : LEOEC_E_BAD_SIZE;
}

// ---------------------------------------------------------------------------
// The bitmatrix classes: leoec_scrub_ws_dev.

// A cauchyrs or liberation configuration: leoec_locate_ws_dev's statuses (an
// empty batch with no buffers goes through its layout, parameter and served
// tests and ends there: no device), then k + m = 32, where id 31's bit is
// LEOEC_LOCATE_MANY's own and the totals could not be counted.
int bit_scrub_served(int coding, int k, int m, int w, uint64_t size) {
  const int rc = op_locate_ws_dev(coding, k, m, w, nullptr, 0, size, 0, nullptr, 0, nullptr, nullptr,
                                  0, nullptr, nullptr);
  if (rc) return rc;
  return scrub_bit_shape(k, m, w);
}

int scrub_bit_fn(const Code& c, const int* surv, int block, std::vector<uint8_t>* rows) {
  return bit_rows(c, surv, &block, 1, rows);
}

// The block table of the code on the current device (dev_table.hpp), one per
// (coding, k, m, w, device), in a cache of their own beside heal's pattern
// tables: nullptr when it is full, and the caller runs the composition.
int scrub_bit_table(const Code& c, const uint32_t** out) {
  // at most 16 x 95 KB of device memory; leaked: never destroyed at exit
  static auto* const cache = new DevTableCache<std::tuple<int, int, int, int>, 16>;
  const auto rows = [&c](const int* surv, int block, std::vector<uint8_t>* r) {
    return scrub_bit_fn(c, surv, block, r);
  };
  const auto build = [&](std::vector<uint32_t>* host) {
    return scrub_bit_build_table(c.k, c.m, c.w, rows, host);
  };
  return cache->get(std::make_tuple(c.coding, c.k, c.m, c.w), build, out);
}

// Header and index words for nobj objects plus an encode region of `enc`
// bytes; false when that overflows.
bool scrub_ws_workspace(uint64_t nobj, uint64_t enc, uint64_t* bytes) {
  uint64_t head;
  return scrub_workspace(nobj, &head) && !__builtin_add_overflow(head, enc, bytes);
}

int op_scrub_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                              uint64_t* bytes) {
  if (!bit_class(coding)) return op_scrub_dev_workspace(coding, k, m, w, size, nobj, bytes);
  int rc = bit_scrub_served(coding, k, m, w, size);
  if (rc) return rc;
  if (!bytes) return LEOEC_E_ARG;
  uint64_t bs = 0, enc;
  if ((rc = op_layout(coding, k, m, w, size, &bs, nullptr))) return rc;
  if (!encode_region_bytes(m, bs, nobj, &enc)) return LEOEC_E_BAD_SIZE;
  return scrub_ws_workspace(nobj, enc, bytes) ? LEOEC_OK : LEOEC_E_BAD_SIZE;
}

// ---------------------------------------------------------------------------
// The GF(2^w) word classes: leoec_scrub_gfw_dev.

// A configuration of class (c): leoec_locate_gfw_dev's statuses (an empty
// batch with no buffers goes through its layout, parameter and served tests
// and ends there: no device), then k + m = 32, for bit_scrub_served's reason.
int gfw_scrub_served(int coding, int k, int m, int w, uint64_t size) {
  const int rc = op_locate_gfw_dev(coding, k, m, w, nullptr, 0, size, 0, nullptr, 0, nullptr,
                                   nullptr, 0, nullptr, nullptr);
  if (rc) return rc;
  return scrub_gfw_shape(k, m);
}

// The host image of a code's block table, built once and kept with the cached
// Code (get_code never frees one); needs no device.  The device gets a copy of
// it (scrub_gfw_table), leoec_scrub_wrows reads its records.
int scrub_gfw_image(const Code* c, const std::vector<uint32_t>** out) {
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
    const auto rows = [c](const int* surv, int block, std::vector<uint32_t>* r) {
      return gf_rows(*c, surv, &block, 1, r);
    };
    e.rc = scrub_gfw_build_table(c->k, c->m, rows, &e.image);
    it = cache.emplace(c, std::move(e)).first;
  }
  *out = &it->second.image;
  return it->second.rc;
}

// The block table of the code on the current device (dev_table.hpp), one per
// (coding, k, m, w, device), in a cache of its own: nullptr when it is full,
// and the caller runs the composition.
int scrub_gfw_table(const Code& c, const uint32_t** out) {
  // at most 16 x 5 KB of device memory; leaked: never destroyed at exit
  static auto* const cache = new DevTableCache<std::tuple<int, int, int, int>, 16>;
  const auto build = [&](std::vector<uint32_t>* host) {
    const std::vector<uint32_t>* image;
    const int rc = scrub_gfw_image(&c, &image);
    if (!rc) *host = *image;
    return rc;
  };
  return cache->get(std::make_tuple(c.coding, c.k, c.m, c.w), build, out);
}

int op_scrub_gfw_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                               uint64_t* bytes) {
  if (gfw_forwarded(coding, k, m, w))  // its own statuses, layout and parameters first
    return op_scrub_ws_dev_workspace(coding, k, m, w, size, nobj, bytes);
  uint64_t bs = 0;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if ((rc = gfw_scrub_served(coding, k, m, w, size))) return rc;
  if (!bytes) return LEOEC_E_ARG;
  uint64_t enc;
  if (!encode_region_bytes(m, bs, nobj, &enc)) return LEOEC_E_BAD_SIZE;
  return scrub_ws_workspace(nobj, enc, bytes) ? LEOEC_OK : LEOEC_E_BAD_SIZE;
}

// ---------------------------------------------------------------------------
// All three calls.

// The kernel family of a scrub call: leoec_scrub_dev's fused GF(2^8) classes,
// leoec_scrub_ws_dev's bitmatrix classes, leoec_scrub_gfw_dev's word classes.
enum class ScrubKind { gf8, bit, gfw };

// The scrub calls' share of the locate call they run (scrub_steps.hpp):
// leoec_scrub_dev's of op_locate_dev, leoec_scrub_ws_dev's of
// op_locate_ws_dev's bitmatrix branch and leoec_scrub_gfw_dev's of
// op_locate_gfw_dev's word branch.
struct ScrubSteps final : LocateSteps {
  ScrubKind kind = ScrubKind::gf8;
  int k = 0, m = 0, w = 0;
  uint8_t* objs = nullptr;
  uint64_t obj_stride = 0, size = 0, bs = 0, nobj = 0;
  uint8_t* parity = nullptr;
  uint64_t parity_stride = 0;
  uint32_t* report = nullptr;
  uint32_t* totals = nullptr;
  void* workspace = nullptr;
  uint64_t workspace_bytes = 0;
  bool begun = false;               // begin() ran: the device is open
  const uint32_t* table = nullptr;  // heal's; bit, gfw: the block table; nullptr after begin(): cache full
  HealListFn heal = nullptr;        // gf8

  uint32_t* header() const { return static_cast<uint32_t*>(workspace); }
  uint32_t* list() const { return header() + kScrubHeader / sizeof(uint32_t); }

  int check(uint64_t block_size) override {
    bs = block_size;
    if (!totals || ((uintptr_t)totals & 3u)) return LEOEC_E_ARG;
    if (!workspace || ((uintptr_t)workspace & 15u)) return LEOEC_E_ARG;
    uint64_t enc = 0, need;  // the header and the index words; bit, gfw: and one object's encode
    if ((kind != ScrubKind::gf8 && !encode_region_bytes(m, bs, 1, &enc)) ||
        !scrub_ws_workspace(nobj, enc, &need))
      return LEOEC_E_BAD_SIZE;
    if (workspace_bytes < need) return LEOEC_E_ARG;
    if (overlaps(report, nobj * sizeof(uint32_t), workspace, workspace_bytes) ||
        overlaps(totals, 2 * sizeof(uint32_t), workspace, workspace_bytes))
      return LEOEC_E_ARG;
    return LEOEC_OK;
  }

  int begin(const Code& c, hipStream_t s) override {
    const int rc = kind == ScrubKind::bit   ? scrub_bit_table(c, &table)
                   : kind == ScrubKind::gfw ? scrub_gfw_table(c, &table)
                                            : heal_table(c, &table);
    if (rc) return rc;
    begun = true;
    if (kind == ScrubKind::gf8) heal = gf8_heal_list_pick(std::make_index_sequence<kMaxK>{}, k);
    return hipMemsetAsync(totals, 0, 2 * sizeof(uint32_t), s) == hipSuccess ? LEOEC_OK : LEOEC_E_HIP;
  }

  int finish(uint64_t o0, uint64_t no, hipStream_t s) override {
    uint32_t* const words = report + o0;
    if (table && hipMemsetAsync(header(), 0, kScrubHeader, s) != hipSuccess) return LEOEC_E_HIP;
    // no <= 2^31 - 1 words: one grid
    if (launch_kernel(scrub_finish, dim3((uint32_t)((no + kThreads - 1) / kThreads)),
                      dim3(kThreads), 0, s, words, (uint32_t)no, table ? list() : nullptr, header(),
                      totals) != LEOEC_OK)
      return LEOEC_E_HIP;
    if (!table) return LEOEC_OK;
    HealArgs h;
    h.objs = objs + o0 * obj_stride;
    h.obj_stride = obj_stride;
    h.parity = parity + o0 * parity_stride;
    h.parity_stride = parity_stride;
    h.lost = words;
    h.unhealed = nullptr;
    h.table = table;
    h.size = size;
    h.bs = (uint32_t)bs;  // < 2^32 (check_dev_batch); bit, gfw: a multiple of 16 w
    h.k = (uint32_t)k;
    h.m = (uint32_t)m;
    h.nobj = (uint32_t)no;
    h.tiles = h.tmap = h.tperm = 0;  // the launcher's
    const uint32_t cap = kMeasureBuild && knobs().scrub_grid > 0 ? (uint32_t)knobs().scrub_grid : 0u;
    if (kind == ScrubKind::gf8) return heal(h, list(), header(), cap, s);
    if (kind == ScrubKind::gfw) {
      GfwHealArgs g;
      g.h = h;
      g.h.tiles = (uint32_t)((bs + kGfwHealTile - 1) / kGfwHealTile);  // gfw_locate's: no x tiles < 2^31
      g.rec_words = scrub_gfw_record_words(k);
      g.red = field(8).mul(0x80u, 2u);  // alpha^8 reduced: the polynomial's low byte
      return launch_gfw_heal_list(w, g, list(), header(), cap, s);
    }
    BitHealArgs a;
    a.h = h;
    a.w = (uint32_t)w;
    a.ps = (uint32_t)(bs / (uint64_t)w);
    a.h.tiles = (a.ps + kBitHealTile - 1u) / kBitHealTile;  // bit_locate's: no x tiles < 2^31
    a.rec_words = scrub_bit_record_words(k, w);
    a.pad = 0;
    return launch_bit_heal_list(a, list(), header(), cap, s);
  }
};

// The three calls after their own served tests: the locate call with the steps
// in it, then, when the table cache was full, leoec_heal_dev's generic path.
int scrub_run(ScrubKind kind, int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
              uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
              uint32_t* report, uint32_t* totals, void* workspace, uint64_t workspace_bytes,
              hipStream_t s) {
  ScrubSteps st;
  st.kind = kind;
  st.k = k;
  st.m = m;
  st.w = w;
  st.objs = objs;
  st.obj_stride = obj_stride;
  st.size = size;
  st.nobj = nobj;
  st.parity = parity;
  st.parity_stride = parity_stride;
  st.report = report;
  st.totals = totals;
  st.workspace = workspace;
  st.workspace_bytes = workspace_bytes;
  // bit, gfw: the encode region behind the header and the index words (check()
  // refuses a workspace that has none before anything looks at it)
  uint64_t head;
  void* enc = nullptr;
  uint64_t enc_bytes = 0;
  if (kind != ScrubKind::gf8 && workspace && scrub_workspace(nobj, &head) && workspace_bytes > head) {
    enc = static_cast<uint8_t*>(workspace) + head;
    enc_bytes = workspace_bytes - head;
  }
  const int rc =
      kind == ScrubKind::bit   ? op_locate_ws_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                                  parity_stride, report, enc, enc_bytes, s, &st)
      : kind == ScrubKind::gfw ? op_locate_gfw_dev(coding, k, m, w, objs, obj_stride, size, nobj,
                                                   parity, parity_stride, report, enc, enc_bytes, s,
                                                   &st)
                               : op_locate_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                               parity_stride, report, s, &st);
  if (rc || !st.begun || st.table) return rc;
  // the table cache is full: the words are final and counted; the rest is
  // leoec_heal_dev's generic path (one synchronisation)
  return op_heal_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, report,
                     st.list(), s);
}

int op_scrub_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride, uint64_t size,
                 uint64_t nobj, uint8_t* parity, uint64_t parity_stride, uint32_t* report,
                 uint32_t* totals, void* workspace, uint64_t workspace_bytes, hipStream_t s) {
  return scrub_run(ScrubKind::gf8, coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                   report, totals, workspace, workspace_bytes, s);
}

int op_scrub_ws_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                    uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                    uint32_t* report, uint32_t* totals, void* workspace, uint64_t workspace_bytes,
                    hipStream_t s) {
  if (!bit_class(coding))  // served or LEOEC_E_UNSUPPORTED there
    return op_scrub_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride, report,
                        totals, workspace, workspace_bytes, s);
  const int rc = bit_scrub_served(coding, k, m, w, size);
  if (rc) return rc;
  return scrub_run(ScrubKind::bit, coding, k, m, w, objs, obj_stride, size, nobj, parity,
                   parity_stride, report, totals, workspace, workspace_bytes, s);
}

int op_scrub_gfw_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                     uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                     uint32_t* report, uint32_t* totals, void* workspace, uint64_t workspace_bytes,
                     hipStream_t s) {
  if (gfw_forwarded(coding, k, m, w))  // served or LEOEC_E_UNSUPPORTED there
    return op_scrub_ws_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                           report, totals, workspace, workspace_bytes, s);
  const int rc = gfw_scrub_served(coding, k, m, w, size);
  if (rc) return rc;
  return scrub_run(ScrubKind::gfw, coding, k, m, w, objs, obj_stride, size, nobj, parity,
                   parity_stride, report, totals, workspace, workspace_bytes, s);
}

int op_scrub_wrows(int coding, int k, int m, int w, int block, int* surv, uint32_t* coef, int cap) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (gfw_forwarded(coding, k, m, w)) return LEOEC_E_UNSUPPORTED;
  if ((rc = gfw_scrub_served(coding, k, m, w, 0))) return rc;
  if (block < 0 || block >= k + m) return LEOEC_E_BAD_ID;
  if (!surv || !coef || cap < k) return LEOEC_E_ARG;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  const std::vector<uint32_t>* image;
  if ((rc = scrub_gfw_image(c, &image))) return rc;
  return scrub_gfw_record(*image, k, m, block, surv, coef);
}

int op_scrub_bitrows(int coding, int k, int m, int w, int block, int* surv, uint32_t* rows,
                     int cap) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (!bit_class(coding)) return LEOEC_E_UNSUPPORTED;
  if ((rc = bit_scrub_served(coding, k, m, w, 0))) return rc;
  if (block < 0 || block >= k + m) return LEOEC_E_BAD_ID;
  if (!surv || !rows || cap < w * scrub_bit_row_words(k, w)) return LEOEC_E_ARG;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  std::vector<int> sv(k);
  std::vector<uint32_t> t;
  rc = scrub_bit_rows(
      k, m, w, block,
      [c](const int* s, int b, std::vector<uint8_t>* out) { return scrub_bit_fn(*c, s, b, out); },
      sv.data(), &t);
  if (rc) return rc;
  for (int i = 0; i < k; ++i) surv[i] = sv[i];
  for (size_t i = 0; i < t.size(); ++i) rows[i] = t[i];
  return LEOEC_OK;
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_scrub_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                              uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_scrub_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_scrub_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                    uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                    uint32_t* report, uint32_t* totals, void* workspace, uint64_t workspace_bytes,
                    void* stream) {
  return leoec::guarded([&] {
    return leoec::op_scrub_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                               report, totals, workspace, workspace_bytes, (hipStream_t)stream);
  });
}

int leoec_scrub_ws_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                 uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_scrub_ws_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_scrub_ws_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                       uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                       uint32_t* report, uint32_t* totals, void* workspace,
                       uint64_t workspace_bytes, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_scrub_ws_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                  parity_stride, report, totals, workspace, workspace_bytes,
                                  (hipStream_t)stream);
  });
}

int leoec_scrub_bitrows(int coding, int k, int m, int w, int block, int* surv, uint32_t* rows,
                        int cap) {
  return leoec::guarded(
      [&] { return leoec::op_scrub_bitrows(coding, k, m, w, block, surv, rows, cap); });
}

int leoec_scrub_gfw_dev_workspace(int coding, int k, int m, int w, uint64_t size, uint64_t nobj,
                                  uint64_t* bytes) {
  return leoec::guarded(
      [&] { return leoec::op_scrub_gfw_dev_workspace(coding, k, m, w, size, nobj, bytes); });
}

int leoec_scrub_gfw_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                        uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                        uint32_t* report, uint32_t* totals, void* workspace,
                        uint64_t workspace_bytes, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_scrub_gfw_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity,
                                   parity_stride, report, totals, workspace, workspace_bytes,
                                   (hipStream_t)stream);
  });
}

int leoec_scrub_wrows(int coding, int k, int m, int w, int block, int* surv, uint32_t* coef,
                      int cap) {
  return leoec::guarded(
      [&] { return leoec::op_scrub_wrows(coding, k, m, w, block, surv, coef, cap); });
}

}  // extern "C"
