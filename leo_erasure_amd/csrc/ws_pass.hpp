// ws_pass.hpp — the chunked encode pass of the calls that compare a batch's
// stored coding blocks with freshly encoded ones (verify.hip's two-pass path,
// locate.hip's bitmatrix and word classes, and scrub.hip through the former):
// the ordinary encode plan into the caller's workspace, m bs bytes per object
// (object o of a chunk at o * m bs, coding block i at i * bs), then the
// caller's own launches on those rows, a chunk of objects at a time in stream
// order.  Three places, because the callers have statuses and enqueues of
// their own between them: check (needs no device), prepare, run.
#pragma once

#include <memory>
#include <vector>

#include "engine.hpp"
#include "kernels_impl.hpp"

namespace leoec {

// m * bs * nobj, the encode region of a whole batch; false, and *bytes as it
// was, when that overflows.
inline bool encode_region_bytes(int m, uint64_t bs, uint64_t nobj, uint64_t* bytes) {
  uint64_t per, all;
  if (__builtin_mul_overflow((uint64_t)m, bs, &per) || __builtin_mul_overflow(per, nobj, &all))
    return false;
  *bytes = all;
  return true;
}

struct WsPass {
  EncodeShards sh;
  std::shared_ptr<const Plan> plan;
  uint64_t bs = 0, obj_stride = 0;
  int m = 0;

  // The workspace argument: room for one object at least (after
  // check_dev_batch: m * bs cannot overflow).
  static int check(const void* workspace, uint64_t workspace_bytes, int m, uint64_t bs) {
    if (!workspace || ((uintptr_t)workspace & 15u) || workspace_bytes < (uint64_t)m * bs)
      return LEOEC_E_ARG;
    return LEOEC_OK;
  }

  // The batch's shards and its encode plan; nothing enqueued.
  int prepare(const Code& c, uint64_t block_size, uint64_t size, const uint8_t* objs,
              uint64_t stride, const uint8_t* parity, uint64_t parity_stride) {
    bs = block_size;
    obj_stride = stride;
    m = c.m;
    sh = encode_shards(c.k, m, bs, size, objs, stride, parity, parity_stride);
    return make_plan(c, sh.surv(), sh.want(), m, &plan);
  }

  // chunk(o0, no) -> status, after the encode of objects [o0, o0 + no) into
  // the workspace.  groups: workgroups per object of the caller's largest
  // grid.  No grid above 2^31 - 1 workgroups: the caller's, and
  // verify_compare's (m 4 KiB tiles of every block), which keeps the encode
  // plan's launches within theirs.
  template <class F>
  int run(void* workspace, uint64_t workspace_bytes, uint64_t nobj, uint64_t groups, hipStream_t s,
          F&& chunk) const {
    const uint64_t per = (uint64_t)m * bs;  // workspace bytes of one object
    const uint64_t cmp = (uint64_t)m * ((bs + detail::kTileBytes - 1) / detail::kTileBytes);
    const uint64_t max_obj = (uint64_t)0x7FFFFFFF / (groups > cmp ? groups : cmp);
    if (max_obj == 0) return LEOEC_E_BAD_SIZE;
    uint64_t step = workspace_bytes / per;  // objects per pass (>= 1)
    if (step > max_obj) step = max_obj;
    const uint8_t* const ws = static_cast<const uint8_t*>(workspace);
    std::vector<Shard> enc(m);
    for (int i = 0; i < m; ++i) enc[i] = Shard{ws + (uint64_t)i * bs, per, bs};
    for (uint64_t o0 = 0; o0 < nobj; o0 += step) {
      const uint64_t no = nobj - o0 < step ? nobj - o0 : step;
      std::vector<Shard> cin(sh.in);
      for (Shard& x : cin) x.base += o0 * obj_stride;
      int rc = run_plan(*plan, cin, enc, bs, no, s);
      if (rc || (rc = chunk(o0, no))) return rc;
    }
    return LEOEC_OK;
  }
};

}  // namespace leoec
