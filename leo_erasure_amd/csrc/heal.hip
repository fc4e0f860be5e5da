// heal.hip — leoec_heal_dev: rebuild, in place, the blocks each object of a
// device batch has lost, every object with its own set of lost ids (one mask
// word per object), and leoec_heal_rows, the map the engine uses for a mask.
//
// Two paths:
//   fused    GF(2^8) matrix codes with k <= 16, m <= 4 (vandrs w = 8, isars):
//            gf8_heal (heal_impl.hpp), one launch over the whole batch, the
//            survivors, outputs and tables of every object taken from the
//            code's pattern table (heal_table.hpp) on the device, cached
//            per (code, device) (dev_table.hpp); never synchronises;
//   generic  everything else: the masks come back to the host (one stream
//            synchronisation), and every run of consecutive objects with the
//            same mask goes through the ordinary plan of that erasure.
// This unit is kept out of engine.cpp / capi.cpp for verify.hip's reason: the
// host sanitizer harness links those against stand-in kernels.  The gf_init
// warm-up does not load this unit's kernels either.
#include <memory>
#include <tuple>
#include <utility>
#include <vector>

#include "dev_table.hpp"
#include "engine.hpp"
#include "heal_impl.hpp"
#include "knobs.hpp"
#include "scrub_steps.hpp"

namespace leoec {

using namespace detail;

namespace {

template <std::size_t... I>
HealFn gf8_heal_pick(std::index_sequence<I...>, int k) {
  static HealFn (*const sel[])() = {&gf8_heal_launcher<(int)I + 1>...};
  return sel[k - 1]();
}

}  // namespace

// The pattern table of the code on the current device (dev_table.hpp), one per
// (coding, k, m, device): nullptr when the cache is full, and the caller takes
// the generic path.
int heal_table(const Code& c, const uint32_t** out) {
  // at most 16 x 8 MB of device memory; leaked: never destroyed at exit
  static auto* const cache = new DevTableCache<std::tuple<int, int, int>, 16>;
  const auto rows = [&c](const int* surv, const int* want, int nwant, std::vector<uint32_t>* r) {
    return gf_rows(c, surv, want, nwant, r);
  };
  const auto build = [&](std::vector<uint32_t>* host) {
    return heal_build_table(c.k, c.m, rows, host);
  };
  return cache->get(std::make_tuple(c.coding, c.k, c.m), build, out);
}

namespace {

bool recoverable(uint32_t mask, int k, int m) {
  return __builtin_popcount(mask) <= m && ((uint64_t)mask >> (k + m)) == 0;
}

// Generic path: the masks on the host, one plan launch per run.
int heal_generic(const Code& c, uint8_t* objs, uint64_t obj_stride, uint64_t size, uint64_t bs,
                 uint64_t nobj, uint8_t* parity, uint64_t parity_stride, const uint32_t* lost,
                 uint32_t* unhealed, hipStream_t s) {
  const int k = c.k, m = c.m;
  std::vector<uint32_t> mask(nobj), left(nobj);
  if (hipMemcpyAsync(mask.data(), lost, nobj * sizeof(uint32_t), hipMemcpyDeviceToHost, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return LEOEC_E_HIP;
  for (uint64_t o = 0; o < nobj; ++o) left[o] = recoverable(mask[o], k, m) ? 0u : mask[o];
  // (a copy from pageable memory is staged before the call returns: `left`
  // may go out of scope)
  if (hipMemcpyAsync(unhealed, left.data(), nobj * sizeof(uint32_t), hipMemcpyHostToDevice, s) !=
      hipSuccess)
    return LEOEC_E_HIP;
  std::vector<int> surv(k), want(k + m);
  std::vector<Shard> in(k), out;
  for (uint64_t o0 = 0; o0 < nobj;) {
    uint64_t o1 = o0 + 1;
    while (o1 < nobj && mask[o1] == mask[o0]) ++o1;
    const uint32_t mk = mask[o0];
    const uint64_t first = o0, no = o1 - o0;
    o0 = o1;
    if (mk == 0 || !recoverable(mk, k, m)) continue;
    heal_split(k, m, mk, surv.data(), want.data());
    const uint8_t* const ob = objs + first * obj_stride;
    const uint8_t* const pb = parity + first * parity_stride;
    for (int i = 0; i < k; ++i)
      in[i] = block_shard(surv[i], k, bs, size, ob, obj_stride, pb, parity_stride);
    std::vector<int> ids;  // the lost ids with bytes to rebuild
    out.clear();
    for (int x = 0; x < __builtin_popcount(mk); ++x) {
      const int id = want[x];
      // a data block wholly past `size`: nothing to write (as op_decode_dev)
      if (id < k && (uint64_t)id * bs >= size) continue;
      out.push_back(block_shard(id, k, bs, size, ob, obj_stride, pb, parity_stride));
      ids.push_back(id);
    }
    if (ids.empty()) continue;
    std::shared_ptr<const Plan> plan;
    int rc = make_plan(c, surv.data(), ids.data(), (int)ids.size(), &plan);
    if (rc) return rc;
    if ((rc = run_plan(*plan, in, out, bs, no, s))) return rc;
  }
  return LEOEC_OK;
}

}  // namespace

int op_heal_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride, uint64_t size,
                uint64_t nobj, uint8_t* parity, uint64_t parity_stride, const uint32_t* lost,
                uint32_t* unhealed, hipStream_t s) {
  uint64_t bs;
  int rc = op_layout(coding, k, m, w, size, &bs, nullptr);
  if (rc) return rc;
  if (k + m > kHealMaxIds) return LEOEC_E_UNSUPPORTED;
  if (nobj == 0 || bs == 0) return LEOEC_OK;
  if (!lost || !unhealed || lost == unhealed) return LEOEC_E_ARG;
  if (((uintptr_t)lost & 3u) || ((uintptr_t)unhealed & 3u)) return LEOEC_E_ARG;
  if ((rc = check_dev_batch(objs, obj_stride, size, parity, parity_stride, m, bs))) return rc;
  if ((rc = device_init())) return rc;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  const uint32_t* table = nullptr;
  if (gf8_fused_config(coding, k, m, w) && !(kMeasureBuild && knobs().heal_form == 1)) {
    if ((rc = heal_table(*c, &table))) return rc;
  }
  if (!table)
    return heal_generic(*c, objs, obj_stride, size, bs, nobj, parity, parity_stride, lost, unhealed,
                        s);
  const HealFn fn = gf8_heal_pick(std::make_index_sequence<kMaxK>{}, k);
  const uint64_t max_obj = gf8_max_objects(bs);
  for (uint64_t o0 = 0; o0 < nobj; o0 += max_obj) {
    HealArgs a;
    a.objs = objs + o0 * obj_stride;
    a.obj_stride = obj_stride;
    a.parity = parity + o0 * parity_stride;
    a.parity_stride = parity_stride;
    a.lost = lost + o0;
    a.unhealed = unhealed + o0;
    a.table = table;
    a.size = size;
    a.bs = (uint32_t)bs;
    a.k = (uint32_t)k;
    a.m = (uint32_t)m;
    a.nobj = (uint32_t)(nobj - o0 < max_obj ? nobj - o0 : max_obj);
    a.tiles = a.tmap = a.tperm = 0;  // the launcher's
    if ((rc = fn(a, s))) return rc;
  }
  return LEOEC_OK;
}

namespace {

int op_heal_rows(int coding, int k, int m, int w, uint32_t lost_mask, int* surv, int* want,
                 int* nwant, uint32_t* coef, int cap, int* index) {
  int rc = check_params(coding, k, m, w);
  if (rc) return rc;
  if (k + m > kHealMaxIds) return LEOEC_E_UNSUPPORTED;
  const Code* c;
  if ((rc = get_code(coding, k, m, w, &c))) return rc;
  if (((uint64_t)lost_mask >> (k + m)) != 0) return LEOEC_E_BAD_ID;
  const int bits = __builtin_popcount(lost_mask);
  if (bits > m) return LEOEC_E_NOT_ENOUGH_BLOCKS;
  if (!surv || !want || !nwant) return LEOEC_E_ARG;
  std::vector<int> sv(k), wt(k + m);
  heal_split(k, m, lost_mask, sv.data(), wt.data());
  for (int i = 0; i < k; ++i) surv[i] = sv[i];
  for (int i = 0; i < bits; ++i) want[i] = wt[i];
  *nwant = bits;
  if (index)
    *index = bits && gf8_fused_config(coding, k, m, w) ? (int)heal_rank(k, m, lost_mask) : -1;
  if (coef && bits) {
    if (c->C.a.empty()) return LEOEC_E_UNSUPPORTED;  // liberation: no GF(2^w) matrix
    if (cap < bits * k) return LEOEC_E_ARG;
    std::vector<uint32_t> rows;
    if ((rc = gf_rows(*c, sv.data(), wt.data(), bits, &rows))) return rc;
    for (int i = 0; i < bits * k; ++i) coef[i] = rows[i];
  }
  return LEOEC_OK;
}

}  // namespace
}  // namespace leoec

extern "C" {

int leoec_heal_dev(int coding, int k, int m, int w, uint8_t* objs, uint64_t obj_stride,
                   uint64_t size, uint64_t nobj, uint8_t* parity, uint64_t parity_stride,
                   const uint32_t* lost, uint32_t* unhealed, void* stream) {
  return leoec::guarded([&] {
    return leoec::op_heal_dev(coding, k, m, w, objs, obj_stride, size, nobj, parity, parity_stride,
                              lost, unhealed, (hipStream_t)stream);
  });
}

int leoec_heal_rows(int coding, int k, int m, int w, uint32_t lost_mask, int* surv, int* want,
                    int* nwant, uint32_t* coef, int cap, int* index) {
  return leoec::guarded([&] {
    return leoec::op_heal_rows(coding, k, m, w, lost_mask, surv, want, nwant, coef, cap, index);
  });
}

}  // extern "C"
